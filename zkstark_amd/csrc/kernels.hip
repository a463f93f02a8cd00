// kernels.hip -- hand-written gfx950 kernels for the STARK-101 prover hot path.
//
//   ntt_pass_kernel      LDS-tiled radix-2^k NTT passes (replaces polynomial.rs:337-383 lagrange
//                        and polynomial.rs:49-56 solve as used at prover.rs:60-70)
//   compose_kernel       pointwise constraint composition (prover.rs:101-173)
//   fri_fold_kernel      evaluation-form FRI fold (polynomial.rs:385-400 + prover.rs:204-211)
//   fri_final_poly_kernel  coefficients of the layer an early-stopped FRI ends at (one workgroup, inverse NTT in LDS)
//   fri_final_poly_batch_kernel  the same for a proof-major batch: 4096 / M layers per workgroup, compact [1 + 2^D] output
//   merkle_*_kernel      SHA-256 Merkle heap (merkle.rs:14-51)
//   b2s_subtree_kernel   the throughput launches of a BLAKE2s-256 heap (blake2s.hpp)
//   gather_kernel        decommitment gather (merkle.rs:54-71, prover.rs:266-289)
//
// All bulk data is canonical u32 residues; all constants are in Montgomery form (field.hpp).
// No MFMA anywhere: butterflies and SHA rounds are not a dense contraction.
#include "kernels.hpp"

#include <cstdlib>

#include "blake2s.hpp"
#include "field.hpp"
#include "fieldhash_f64.hpp"
#include "sha256_quad.hpp"
#include "sha256.hpp"

namespace zk {

__device__ __forceinline__ uint32_t pow_lookup(const PowTable& t, uint32_t e) {
    return mont_mul(t.hi[e >> t.lo_bits], t.lo[e & ((1u << t.lo_bits) - 1u)]);
}

constexpr uint32_t R2_MONT = R2;   // 2^64 mod P (fieldhash.hpp): canonical -> Montgomery

// Montgomery-domain inverse by Fermat: a^(P-2), P-2 = 0xBFFFFFFF.
__device__ uint32_t mont_inv(uint32_t a) {
    uint32_t r = R1, b = a;
    uint32_t e = P - 2;
#pragma unroll 1
    for (int i = 0; i < 32; ++i) {
        if (e & 1) r = mont_mul(r, b);
        b = mont_mul(b, b);
        e >>= 1;
    }
    return r;
}

// ===========================================================================
// NTT passes
// ===========================================================================
//
// Generic pass for any radix and size (the full-size tiles with R = 64/128/256 take the
// register-radix kernel of ntt_fast.hip instead; this one serves small transforms and odd radices).
// The array is viewed as [A][R][S] with S fastest.  A workgroup owns a tile of C
// columns (a, s) and all R rows t of those columns, stages it in LDS with row
// pitch C+1, runs the log2(R) radix-2 stages there and writes the tile back in
// place.  Global accesses are rows of C contiguous words (C*4 >= 128 B whenever
// S >= 32), or one fully contiguous block when S < C.
//
// Inverse transforms run decimation-in-frequency (natural -> digit-reversed
// order), forward transforms decimation-in-time (digit-reversed -> natural), with
// the same radix list, so iNTT followed by NTT never needs a permutation pass.
// Bit reversal inside one radix-R block is absorbed into the LDS row index.

constexpr int kNttThreads = 256;

__device__ __forceinline__ void tile_coords(uint32_t l, uint32_t logR, uint32_t logS, uint32_t logC,
                                            uint32_t& t, uint32_t& c) {
    if (logS >= logC) {            // row of C contiguous words
        t = l >> logC;
        c = l & ((1u << logC) - 1u);
    } else {                       // whole tile is one contiguous block
        uint32_t s = l & ((1u << logS) - 1u);
        t = (l >> logS) & ((1u << logR) - 1u);
        c = ((l >> (logR + logS)) << logS) | s;
    }
}

template <uint32_t MODE>
__global__ __launch_bounds__(kNttThreads) void ntt_pass_kernel(NttPassArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    p.src += (size_t)blockIdx.y * p.src_stride;      // batch of independent transforms
    p.dst += (size_t)blockIdx.y * p.dst_stride;
    const uint32_t logR = p.logR, logS = p.logS, logC = p.logC;
    const uint32_t R = 1u << logR, C = 1u << logC, pitch = C + 1u;
    uint32_t* tile = smem;              // R * pitch words
    uint32_t* twl = smem + R * pitch;   // R/2 twiddles w_R^j
    const uint32_t tid = threadIdx.x;
    const uint32_t col0 = blockIdx.x << logC;
    const uint32_t tile_elems = R << logC;
    const uint32_t tw_shift = p.L - logR - logS;   // w_{RS} = root^(1 << tw_shift)
    const uint32_t smask = (1u << logS) - 1u;

    for (uint32_t j = tid; j < (R >> 1); j += kNttThreads) twl[j] = pow_lookup(p.tw, j << (p.L - logR));

    // ---- load ---------------------------------------------------------------
    if (MODE == NTT_DIT_LDE) {
        // S = B.  Each (prepared) coefficient feeds B columns: the innermost radix-B stage of the
        // size-N transform sees (c, 0, ..., 0) and is a replication.
        const uint32_t logB = logS;
        const uint32_t a0 = col0 >> logB;
        for (uint32_t u = tid; u < (tile_elems >> logB); u += kNttThreads) {
            uint32_t ao = u >> logR, t = u & (R - 1u);
            uint32_t v = p.src[((size_t)(a0 + ao) << logR) | t];
            uint32_t row = __brev(t) >> (32u - logR);
            uint32_t* dstp = &tile[row * pitch + (ao << logB)];
            dstp[0] = v;
            for (uint32_t s = 1; s <= smask; ++s) dstp[s] = mont_mul(v, pow_lookup(p.tw, (t * s) << tw_shift));
        }
    } else {
        for (uint32_t l = tid; l < tile_elems; l += kNttThreads) {
            uint32_t t, c;
            tile_coords(l, logR, logS, logC, t, c);
            uint32_t col = col0 + c, a = col >> logS, s = col & smask;
            size_t addr = ((size_t)a << (logR + logS)) | ((size_t)t << logS) | s;
            uint32_t v = p.src[addr];
            uint32_t row = t;
            if (MODE == NTT_DIT) {
                if (logS) v = mont_mul(v, pow_lookup(p.tw, (t * s) << tw_shift));
                row = __brev(t) >> (32u - logR);
            }
            tile[row * pitch + c] = v;
        }
    }
    __syncthreads();

    // ---- log2(R) radix-2 stages in LDS ------------------------------------------
    const uint32_t nb = tile_elems >> 1;
    if (MODE == NTT_DIF) {   // Gentleman-Sande: natural in, bit-reversed out
        for (int ll = (int)logR - 1; ll >= 0; --ll) {
            for (uint32_t b = tid; b < nb; b += kNttThreads) {
                uint32_t c = b & (C - 1u), pi = b >> logC;
                uint32_t j = pi & ((1u << ll) - 1u);
                uint32_t i = ((pi >> ll) << (ll + 1)) | j;
                uint32_t* x0 = &tile[i * pitch + c];
                uint32_t* x1 = x0 + (pitch << ll);
                uint32_t u = *x0, v = *x1;
                *x0 = add(u, v);
                *x1 = mont_mul(sub(u, v), twl[j << (logR - 1u - ll)]);
            }
            __syncthreads();
        }
    } else {                 // Cooley-Tukey: bit-reversed in, natural out
        for (uint32_t ll = 0; ll < logR; ++ll) {
            for (uint32_t b = tid; b < nb; b += kNttThreads) {
                uint32_t c = b & (C - 1u), pi = b >> logC;
                uint32_t j = pi & ((1u << ll) - 1u);
                uint32_t i = ((pi >> ll) << (ll + 1)) | j;
                uint32_t* x0 = &tile[i * pitch + c];
                uint32_t* x1 = x0 + (pitch << ll);
                uint32_t u = *x0, v = mont_mul(*x1, twl[j << (logR - 1u - ll)]);
                *x0 = add(u, v);
                *x1 = sub(u, v);
            }
            __syncthreads();
        }
    }

    // ---- store --------------------------------------------------------------
    for (uint32_t l = tid; l < tile_elems; l += kNttThreads) {
        uint32_t t, c;
        tile_coords(l, logR, logS, logC, t, c);
        uint32_t col = col0 + c, a = col >> logS, s = col & smask;
        size_t addr = ((size_t)a << (logR + logS)) | ((size_t)t << logS) | s;
        uint32_t v;
        if (MODE == NTT_DIF) {
            v = tile[(__brev(t) >> (32u - logR)) * pitch + c];
            if (logS) v = mont_mul(v, pow_lookup(p.tw, (t * s) << tw_shift));
            else if (p.scale_mont) v = mont_mul(v, p.scale_mont);
        } else {
            v = tile[t * pitch + c];
        }
        p.dst[addr] = v;
    }
}

bool launch_ntt_pass_fast(const NttPassArgs& a, NttMode mode, hipStream_t s, hipError_t* err);   // ntt_fast.hip

hipError_t launch_ntt_pass(const NttPassArgs& a, NttMode mode, hipStream_t s, Profiler* prof) {
    // algorithmic bytes: every element read once and written once (the LDE pass reads n, writes N)
    double bytes = mode == NTT_DIT_LDE ? 4.0 * ((double)((size_t)1 << (a.log_total - a.logS)) + (double)((size_t)1 << a.log_total))
                                       : 8.0 * (double)((size_t)1 << a.log_total);
    const uint32_t batch = a.batch ? a.batch : 1;
    ScopedKernelTimer tm(prof, K_NTT, bytes * batch, s, kNttOpsPerElement * (double)((size_t)1 << a.log_total) * batch * (double)a.logR / 7.0);
    hipError_t ferr = hipSuccess;
    if (launch_ntt_pass_fast(a, mode, s, &ferr)) return ferr;
    uint32_t cols_log = a.log_total - a.logR;
    uint32_t blocks = 1u << (cols_log - a.logC);
    size_t shmem = ((size_t)(1u << a.logR) * ((1u << a.logC) + 1u) + (1u << a.logR) / 2u) * sizeof(uint32_t);
    switch (mode) {
        case NTT_DIF: hipLaunchKernelGGL(ntt_pass_kernel<NTT_DIF>, dim3(blocks, batch), dim3(kNttThreads), shmem, s, a); break;
        case NTT_DIT: hipLaunchKernelGGL(ntt_pass_kernel<NTT_DIT>, dim3(blocks, batch), dim3(kNttThreads), shmem, s, a); break;
        case NTT_DIT_LDE: hipLaunchKernelGGL(ntt_pass_kernel<NTT_DIT_LDE>, dim3(blocks, batch), dim3(kNttThreads), shmem, s, a); break;
    }
    return hipGetLastError();
}

// Interpolant coefficients for the LDE, from the unscaled DIF output U of (a_0..a_{n-2}, 0):
//   out[pos] = (U[pos] - U[n-1] g^(k+1)) * shift^k / n,   k = true index of storage position pos.
// The first term removes the degree-(n-1) coefficient (the reference interpolates n-1 points,
// prover.rs:60: "virtual last trace point"), shift^k moves to the coset (prover.rs:69).
__global__ __launch_bounds__(256) void coef_prepare_kernel(const uint32_t* U, uint32_t* out, CoefPrepArgs a, size_t u_stride, size_t out_stride) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x, n = 1u << a.log_n;
    if (pos >= n) return;
    U += (size_t)blockIdx.y * u_stride;
    out += (size_t)blockIdx.y * out_stride;
    uint32_t k = 0, rem = a.log_n, sh = 0;
    for (uint32_t d = 0; d < a.nd; ++d) {
        rem -= a.dig_bits[d];
        k |= ((pos >> rem) & ((1u << a.dig_bits[d]) - 1u)) << sh;
        sh += a.dig_bits[d];
    }
    const uint32_t c_top = U[n - 1u];
    uint32_t v = sub(U[pos], mont_mul(c_top, pow_lookup(a.tw, ((k + 1u) & (n - 1u)) << a.log_b)));
    out[pos] = mont_mul(v, mont_mul(pow_lookup(a.wtab, k), a.ninv_mont));
}

hipError_t launch_coef_prepare(const uint32_t* U, uint32_t* out, const CoefPrepArgs& a, hipStream_t s, Profiler* prof,
                               uint32_t batch, size_t u_stride, size_t out_stride) {
    uint32_t n = 1u << a.log_n;
    ScopedKernelTimer tm(prof, K_NTT, 8.0 * n * batch, s);
    hipLaunchKernelGGL(coef_prepare_kernel, dim3((n + 255) / 256, batch), dim3(256), 0, s, U, out, a, u_stride, out_stride);
    return hipGetLastError();
}

struct DigitArgs {
    uint32_t nd;
    uint32_t bits[kMaxDigits];
};

// to_natural: out[true_index(pos)] = in[pos]; else out[pos] = in[true_index(pos)]
__global__ void digit_reverse_kernel(const uint32_t* in, uint32_t* out, uint32_t log_m, DigitArgs dg, int to_natural) {
    size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= ((size_t)1 << log_m)) return;
    uint32_t k = 0, rem = log_m, sh = 0;
    for (uint32_t d = 0; d < dg.nd; ++d) {
        rem -= dg.bits[d];
        k |= (((uint32_t)pos >> rem) & ((1u << dg.bits[d]) - 1u)) << sh;
        sh += dg.bits[d];
    }
    if (to_natural) out[k] = in[pos];
    else out[pos] = in[k];
}

hipError_t launch_digit_reverse(const uint32_t* in, uint32_t* out, uint32_t log_m, uint32_t nd,
                                const uint32_t* dig_bits, int to_natural, hipStream_t s) {
    DigitArgs dg{};
    dg.nd = nd;
    for (uint32_t i = 0; i < nd; ++i) dg.bits[i] = dig_bits[i];
    size_t m = (size_t)1 << log_m;
    uint32_t threads = 256, blocks = (uint32_t)((m + threads - 1) / threads);
    hipLaunchKernelGGL(digit_reverse_kernel, dim3(blocks), dim3(threads), 0, s, in, out, log_m, dg, to_natural);
    return hipGetLastError();
}

// Degree check of the opt-in reference self-checks (prover.rs:154-156, :169, :228-251): coef is the unscaled DIF output
// (mixed-radix digit-reversed order) of a layer; out[0] += number of non-zero coefficients of true index >= bound,
// out[1] = the coefficient of true index bound - 1 (the asserted degree must be reached exactly).
__global__ void degree_check_kernel(const uint32_t* coef, uint32_t log_m, DigitArgs dg, uint32_t bound, uint32_t* out) {
    size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= ((size_t)1 << log_m)) return;
    uint32_t k = 0, rem = log_m, sh = 0;
    for (uint32_t d = 0; d < dg.nd; ++d) {
        rem -= dg.bits[d];
        k |= (((uint32_t)pos >> rem) & ((1u << dg.bits[d]) - 1u)) << sh;
        sh += dg.bits[d];
    }
    const uint32_t v = coef[pos];
    if (k >= bound && v != 0) atomicAdd(&out[0], 1u);
    if (k + 1 == bound) out[1] = v;
}
hipError_t launch_degree_check(const uint32_t* coef, uint32_t log_m, uint32_t nd, const uint32_t* dig_bits, uint32_t bound, uint32_t* out, hipStream_t s) {
    DigitArgs dg{};
    dg.nd = nd;
    for (uint32_t i = 0; i < nd; ++i) dg.bits[i] = dig_bits[i];
    size_t m = (size_t)1 << log_m;
    hipLaunchKernelGGL(degree_check_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, s, coef, log_m, dg, bound, out);
    return hipGetLastError();
}

// ===========================================================================
// Composition
// ===========================================================================

// Domain setup: inv_xm1[i] = 1/(shift h^i - 1), Montgomery form.  Each thread inverts
// kInvBatch denominators with one Fermat inversion (Montgomery's trick).
constexpr int kInvBatch = 8;

__global__ __launch_bounds__(256) void build_inv_xm1_kernel(uint32_t* out, size_t count, uint32_t e0, uint32_t order_mask, PowTable htab, uint32_t w_mont) {
    size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t base = gid * kInvBatch;
    if (base >= count) return;
    uint32_t d[kInvBatch], pre[kInvBatch];
    uint32_t acc = R1;
#pragma unroll
    for (int e = 0; e < kInvBatch; ++e) {
        size_t i = base + e;
        uint32_t x = i < count ? mont_mul(pow_lookup(htab, (e0 + (uint32_t)i) & order_mask), w_mont) : add(R1, R1);
        d[e] = sub(x, R1);
        pre[e] = acc;
        acc = mont_mul(acc, d[e]);
    }
    uint32_t inv = mont_inv(acc);
#pragma unroll
    for (int e = kInvBatch - 1; e >= 0; --e) {
        size_t i = base + e;
        uint32_t r = mont_mul(inv, pre[e]);
        inv = mont_mul(inv, d[e]);
        if (i < count) out[i] = r;
    }
}

hipError_t launch_build_inv_xm1_range(uint32_t* out, size_t count, uint32_t e0, uint32_t log_order, PowTable htab, uint32_t shift_mont, hipStream_t s) {
    size_t threads_total = (count + kInvBatch - 1) / kInvBatch;
    uint32_t blocks = (uint32_t)((threads_total + 255) / 256);
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(build_inv_xm1_kernel, dim3(blocks), dim3(256), 0, s, out, count, e0, (uint32_t)(((uint64_t)1 << log_order) - 1u), htab, shift_mont);
    return hipGetLastError();
}
hipError_t launch_build_inv_xm1(uint32_t* out, uint32_t logN, PowTable htab, uint32_t shift_mont, hipStream_t s) {
    return launch_build_inv_xm1_range(out, (size_t)1 << logN, 0u, logN, htab, shift_mont, s);
}

// cp(x_i) for x_i = w h^i (prover.rs:101-166 evaluated pointwise; the same formula the
// verifier recomputes at proof.rs:63-77):
//   p0 = (f(x) - a[0]) / (x - 1)
//   p1 = (f(x) - a[n-2]) / (x - g^(n-2))            = (f(x) - a[n-2]) * g^2 / (x_{i+2B} - 1)
//   p2 = (f(g^2 x) - f(g x)^2 - f(x)^2) (x - g^(n-3))(x - g^(n-2))(x - g^(n-1)) / (x^n - 1)
//   cp = alpha0 p0 + alpha1 p1 + alpha2 p2
// with f(g x_i) = f[i+B], f(g^2 x_i) = f[i+2B] (indices mod N); x^n - 1 depends on i mod B only.
// BATCH: f and the trace / challenge constants belong to one proof of a batch, and a.zz carries no alpha2.
struct ComposeRaw { uint32_t f0, f1, f2, inv0, inv2, x_hi, x_lo, zz; };
__device__ __forceinline__ ComposeRaw compose_fetch(const ComposeArgs& a, const uint32_t* f, size_t i) {
    const size_t N = (size_t)1 << a.logN;
    const uint32_t B = 1u << a.log_b;
    const size_t i1 = (i + B) & (N - 1), i2 = (i + 2 * (size_t)B) & (N - 1);
    ComposeRaw r;
    r.f0 = f[i]; r.f1 = f[i1]; r.f2 = f[i2];
    r.inv0 = a.inv_xm1[i]; r.inv2 = a.inv_xm1[i2];
    r.x_hi = a.htab.hi[(uint32_t)i >> a.htab.lo_bits]; r.x_lo = a.htab.lo[(uint32_t)i & ((1u << a.htab.lo_bits) - 1u)];   // pow_lookup's two halves
    r.zz = a.zz[i & (B - 1)];
    return r;
}
// one value of cp from its operands: f at the three taps, 1/(x - 1) at two, x itself (Montgomery), zz = alpha2 / (x^n - 1) R^2
template <bool BATCH>
__device__ __forceinline__ uint32_t compose_eval(const ComposeArgs& a, uint32_t f0, uint32_t f1, uint32_t f2, uint32_t inv0, uint32_t inv2,
                                                 uint32_t x, uint32_t zz, uint32_t first, uint32_t last, uint32_t al0, uint32_t al1g2, uint32_t al2) {
    uint32_t t0 = mont_mul(mont_mul(sub(f0, first), inv0), al0);
    uint32_t t1 = mont_mul(mont_mul(sub(f0, last), inv2), al1g2);
    uint32_t v3 = mont_mul(mont_mul(sub(x, a.gm3_mont), sub(x, a.gm2_mont)), sub(x, a.gm1_mont));   // V*R
    uint32_t y = mont_mul(v3, zz);                                               // alpha2 V / (x^n-1) * R^2
    if (BATCH) y = mont_mul(y, al2);
    // data*data products carry R^-1; bring f2 to the same scale, fix with the R^2 in y
    uint32_t num = sub(sub(mont_mul(f2, 1u), mont_mul(f1, f1)), mont_mul(f0, f0));
    uint32_t t2 = mont_mul(num, y);
    return add(add(t0, t1), t2);
}
template <bool BATCH>
__device__ __forceinline__ uint32_t compose_finish(const ComposeArgs& a, const ComposeRaw& r, uint32_t first, uint32_t last, uint32_t al0,
                                                   uint32_t al1g2, uint32_t al2) {
    const uint32_t x = mont_mul(mont_mul(r.x_hi, r.x_lo), a.w_mont);              // Montgomery x_i
    return compose_eval<BATCH>(a, r.f0, r.f1, r.f2, r.inv0, r.inv2, x, r.zz, first, last, al0, al1g2, al2);
}
template <bool BATCH>
__device__ __forceinline__ uint32_t compose_core(const ComposeArgs& a, const uint32_t* f, uint32_t first, uint32_t last, uint32_t al0,
                                                 uint32_t al1g2, uint32_t al2, size_t i) {
    return compose_finish<BATCH>(a, compose_fetch(a, f, i), first, last, al0, al1g2, al2);
}
__device__ __forceinline__ uint32_t compose_at(const ComposeArgs& a, size_t i) {
    return compose_core<false>(a, a.f, a.first, a.last, a.alpha0_mont, a.alpha1g2_mont, 0u, i);
}

__global__ __launch_bounds__(256) void compose_kernel(ComposeArgs a) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ((size_t)1 << a.logN)) return;
    a.cp[i] = compose_at(a, i);
}

// Four consecutive values per thread, 16-byte accesses (the stand-alone stage: HBM-bound, and one value per thread leaves
// the memory system short of requests).  The taps i + B and i + 2B are whole vectors when B >= 4; for B = 1, 2 (the local
// domains of a proof sharded over 8 or 4 GPUs) they are windows of the two vectors at i and i + 4.  x advances by h.
__global__ __launch_bounds__(256) void compose_kernel4(ComposeArgs a) {
    const size_t N = (size_t)1 << a.logN;
    const uint32_t B = 1u << a.log_b;
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= N) return;
    const uint4* fv = reinterpret_cast<const uint4*>(a.f);
    const uint4* iv = reinterpret_cast<const uint4*>(a.inv_xm1);
    uint32_t f0[4], f1[4], f2[4], inv0[4], inv2[4], zz[4];
    const uint4 v0 = fv[i >> 2], w0 = iv[i >> 2];
    f0[0] = v0.x; f0[1] = v0.y; f0[2] = v0.z; f0[3] = v0.w;
    inv0[0] = w0.x; inv0[1] = w0.y; inv0[2] = w0.z; inv0[3] = w0.w;
    if (B >= 4) {
        const uint4 v1 = fv[((i + B) & (N - 1)) >> 2], v2 = fv[((i + 2 * (size_t)B) & (N - 1)) >> 2], w2 = iv[((i + 2 * (size_t)B) & (N - 1)) >> 2];
        f1[0] = v1.x; f1[1] = v1.y; f1[2] = v1.z; f1[3] = v1.w;
        f2[0] = v2.x; f2[1] = v2.y; f2[2] = v2.z; f2[3] = v2.w;
        inv2[0] = w2.x; inv2[1] = w2.y; inv2[2] = w2.z; inv2[3] = w2.w;
        const uint32_t z0 = (uint32_t)i & (B - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) zz[k] = a.zz[z0 + k];
    } else {
        const uint4 v1 = fv[((i + 4) & (N - 1)) >> 2], w1 = iv[((i + 4) & (N - 1)) >> 2];
        const uint32_t fw[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        const uint32_t iw[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f1[k] = B == 1 ? fw[k + 1] : fw[k + 2];
            f2[k] = B == 1 ? fw[k + 2] : fw[k + 4];
            inv2[k] = B == 1 ? iw[k + 2] : iw[k + 4];
            zz[k] = B == 1 ? a.zz[0] : a.zz[k & 1];
        }
    }
    uint32_t x = mont_mul(pow_lookup(a.htab, (uint32_t)i), a.w_mont);
    const uint32_t h = pow_lookup(a.htab, 1u);
    uint32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r[k] = compose_eval<false>(a, f0[k], f1[k], f2[k], inv0[k], inv2[k], x, zz[k], a.first, a.last, a.alpha0_mont, a.alpha1g2_mont, 0u);
        if (k < 3) x = mont_mul(x, h);
    }
    reinterpret_cast<uint4*>(a.cp)[i >> 2] = make_uint4(r[0], r[1], r[2], r[3]);
}

hipError_t launch_compose(const ComposeArgs& a, hipStream_t s, Profiler* prof) {
    size_t N = (size_t)1 << a.logN;
    ScopedKernelTimer tm(prof, K_COMPOSE, 8.0 * (double)N, s);   // read f once, write cp once
    const bool aligned = ((reinterpret_cast<uintptr_t>(a.f) | reinterpret_cast<uintptr_t>(a.inv_xm1) | reinterpret_cast<uintptr_t>(a.cp)) & 15u) == 0;
    if (a.logN >= 4 && aligned) {
        uint32_t blocks = (uint32_t)((N / 4 + 255) / 256);
        hipLaunchKernelGGL(compose_kernel4, dim3(blocks), dim3(256), 0, s, a);
    } else {
        uint32_t blocks = (uint32_t)((N + 255) / 256);
        hipLaunchKernelGGL(compose_kernel, dim3(blocks), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

// ---- cp over E (ComposeExtArgs) ----------------------------------------------------------------------------------
// cp = alpha0 p0 + alpha1 p1 + alpha2 p2 with the alphas in E and p0, p1, p2 in the base field: the operands are fetched once and the
// three quotient terms formed once, then each plane takes its own three products.  compose_eval's t2 = num * (v3 * zz) is taken as
// (num * v3) * zz here -- the same residue, and the product that does not depend on the component is shared -- so a value costs 14
// Montgomery multiplications where compose_eval has 11, and plane j is compose_eval with component j of the alphas word for word.
__device__ __forceinline__ Ext compose_ext_eval(const ComposeExtArgs& e, uint32_t f0, uint32_t f1, uint32_t f2, uint32_t inv0, uint32_t inv2,
                                                    uint32_t x, uint32_t zz0, uint32_t zz1) {
    const ComposeArgs& a = e.a;
    const uint32_t q0 = mont_mul(sub(f0, a.first), inv0);
    const uint32_t q1 = mont_mul(sub(f0, a.last), inv2);
    const uint32_t v3 = mont_mul(mont_mul(sub(x, a.gm3_mont), sub(x, a.gm2_mont)), sub(x, a.gm1_mont));   // V*R
    const uint32_t num = sub(sub(mont_mul(f2, 1u), mont_mul(f1, f1)), mont_mul(f0, f0));
    const uint32_t nv = mont_mul(num, v3);
    Ext r;
    r.c0 = add(add(mont_mul(q0, a.alpha0_mont), mont_mul(q1, a.alpha1g2_mont)), mont_mul(nv, zz0));
    r.c1 = add(add(mont_mul(q0, e.alpha0_mont1), mont_mul(q1, e.alpha1g2_mont1)), mont_mul(nv, zz1));
    return r;
}

__global__ __launch_bounds__(256) void compose_ext_kernel(ComposeExtArgs e) {
    const ComposeArgs& a = e.a;
    const size_t N = (size_t)1 << a.logN;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const ComposeRaw r = compose_fetch(a, a.f, i);
    const uint32_t x = mont_mul(mont_mul(r.x_hi, r.x_lo), a.w_mont);
    const Ext v = compose_ext_eval(e, r.f0, r.f1, r.f2, r.inv0, r.inv2, x, r.zz, e.zz1[i & ((1u << a.log_b) - 1)]);
    a.cp[i] = v.c0;
    a.cp[N + i] = v.c1;
}

// compose_kernel4's fetches and taps (whole vectors for B >= 4, windows for B = 1, 2), one 16-byte store per plane
__global__ __launch_bounds__(256) void compose_ext_kernel4(ComposeExtArgs e) {
    const ComposeArgs& a = e.a;
    const size_t N = (size_t)1 << a.logN;
    const uint32_t B = 1u << a.log_b;
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= N) return;
    const uint4* fv = reinterpret_cast<const uint4*>(a.f);
    const uint4* iv = reinterpret_cast<const uint4*>(a.inv_xm1);
    uint32_t f0[4], f1[4], f2[4], inv0[4], inv2[4], zz0[4], zz1[4];
    const uint4 v0 = fv[i >> 2], w0 = iv[i >> 2];
    f0[0] = v0.x; f0[1] = v0.y; f0[2] = v0.z; f0[3] = v0.w;
    inv0[0] = w0.x; inv0[1] = w0.y; inv0[2] = w0.z; inv0[3] = w0.w;
    if (B >= 4) {
        const uint4 v1 = fv[((i + B) & (N - 1)) >> 2], v2 = fv[((i + 2 * (size_t)B) & (N - 1)) >> 2], w2 = iv[((i + 2 * (size_t)B) & (N - 1)) >> 2];
        f1[0] = v1.x; f1[1] = v1.y; f1[2] = v1.z; f1[3] = v1.w;
        f2[0] = v2.x; f2[1] = v2.y; f2[2] = v2.z; f2[3] = v2.w;
        inv2[0] = w2.x; inv2[1] = w2.y; inv2[2] = w2.z; inv2[3] = w2.w;
        const uint32_t z0 = (uint32_t)i & (B - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) { zz0[k] = a.zz[z0 + k]; zz1[k] = e.zz1[z0 + k]; }
    } else {
        const uint4 v1 = fv[((i + 4) & (N - 1)) >> 2], w1 = iv[((i + 4) & (N - 1)) >> 2];
        const uint32_t fw[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        const uint32_t iw[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f1[k] = B == 1 ? fw[k + 1] : fw[k + 2];
            f2[k] = B == 1 ? fw[k + 2] : fw[k + 4];
            inv2[k] = B == 1 ? iw[k + 2] : iw[k + 4];
            zz0[k] = B == 1 ? a.zz[0] : a.zz[k & 1];
            zz1[k] = B == 1 ? e.zz1[0] : e.zz1[k & 1];
        }
    }
    uint32_t x = mont_mul(pow_lookup(a.htab, (uint32_t)i), a.w_mont);
    const uint32_t h = pow_lookup(a.htab, 1u);
    Ext r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r[k] = compose_ext_eval(e, f0[k], f1[k], f2[k], inv0[k], inv2[k], x, zz0[k], zz1[k]);
        if (k < 3) x = mont_mul(x, h);
    }
    reinterpret_cast<uint4*>(a.cp)[i >> 2] = make_uint4(r[0].c0, r[1].c0, r[2].c0, r[3].c0);
    reinterpret_cast<uint4*>(a.cp)[(N + i) >> 2] = make_uint4(r[0].c1, r[1].c1, r[2].c1, r[3].c1);
}

hipError_t launch_compose_ext(const ComposeExtArgs& e, hipStream_t s, Profiler* prof) {
    const ComposeArgs& a = e.a;
    const size_t N = (size_t)1 << a.logN;
    ScopedKernelTimer tm(prof, K_COMPOSE, 12.0 * (double)N, s);   // read f once, write two planes
    const bool aligned = ((reinterpret_cast<uintptr_t>(a.f) | reinterpret_cast<uintptr_t>(a.inv_xm1) | reinterpret_cast<uintptr_t>(a.cp)) & 15u) == 0;
    if (a.logN >= 4 && aligned) hipLaunchKernelGGL(compose_ext_kernel4, dim3((uint32_t)((N / 4 + 255) / 256)), dim3(256), 0, s, e);
    else hipLaunchKernelGGL(compose_ext_kernel, dim3((uint32_t)((N + 255) / 256)), dim3(256), 0, s, e);
    return hipGetLastError();
}

// cp of a proof-major batch, stored only (the batched prover with coset leaves: the tree over cp then has group 0's cosets as
// leaves, which the fused one-value leaf source cannot hash): value b * N + i = cp_b[i] with proof b's own trace constants and
// challenges, the arithmetic of ComposeBatchSrc.
__global__ __launch_bounds__(256) void compose_batch_kernel(ComposeArgs a, const BatchChal* __restrict__ chal, size_t total) {
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= total) return;
    const size_t b = pos >> a.logN, i = pos & (((size_t)1 << a.logN) - 1);
    const BatchChal c = chal[b];
    a.cp[pos] = compose_core<true>(a, a.f + (b << a.logN), c.first, c.last, c.alpha0_mont, c.alpha1g2_mont, c.alpha2_mont, i);
}
hipError_t launch_compose_batch(const ComposeBatchArgs& a, uint32_t log_batch, hipStream_t s, Profiler* prof) {
    if (!a.chal || a.a.logN + log_batch > 32) return hipErrorInvalidValue;
    const size_t total = (size_t)1 << (a.a.logN + log_batch);
    ScopedKernelTimer tm(prof, K_COMPOSE, 8.0 * (double)total, s);   // read f once, write cp once
    hipLaunchKernelGGL(compose_batch_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, a.a, a.chal, total);
    return hipGetLastError();
}

// ---- cp over E of a proof-major batch (launch_compose_ext_batch) ---------------------------------------------------
// compose_ext_eval with proof b's constants from the two per-proof tables.  a.zz carries no alpha (R^2 / (x^n - 1), as for every batch
// composition), so the component-free product goes one step further, y = (num * v3) * zz, and each plane takes its three products by
// its own alphas: 15 Montgomery multiplications per value, one more than compose_ext_eval, which has alpha2 folded into its two zz
// tables on the host.  Plane j is compose_eval<true> with component j of the alphas, residue for residue.
struct ComposeExtConsts { uint32_t first, last, a0[2], a1g2[2], a2[2]; };
__device__ __forceinline__ ComposeExtConsts compose_ext_batch_consts(const BatchChal* __restrict__ chal, const BatchChalExt* __restrict__ xchal, size_t b) {
    const BatchChal c = chal[b];
    const BatchChalExt x = xchal[b];
    return ComposeExtConsts{c.first, c.last, {c.alpha0_mont, x.alpha0_mont1}, {c.alpha1g2_mont, x.alpha1g2_mont1}, {c.alpha2_mont, x.alpha2_mont1}};
}
__device__ __forceinline__ Ext compose_ext_batch_eval(const ComposeArgs& a, const ComposeExtConsts& k, uint32_t f0, uint32_t f1, uint32_t f2, uint32_t inv0,
                                                      uint32_t inv2, uint32_t x, uint32_t zz) {
    const uint32_t q0 = mont_mul(sub(f0, k.first), inv0);
    const uint32_t q1 = mont_mul(sub(f0, k.last), inv2);
    const uint32_t v3 = mont_mul(mont_mul(sub(x, a.gm3_mont), sub(x, a.gm2_mont)), sub(x, a.gm1_mont));   // V*R
    const uint32_t num = sub(sub(mont_mul(f2, 1u), mont_mul(f1, f1)), mont_mul(f0, f0));
    const uint32_t y = mont_mul(mont_mul(num, v3), zz);
    Ext r;
    r.c0 = add(add(mont_mul(q0, k.a0[0]), mont_mul(q1, k.a1g2[0])), mont_mul(y, k.a2[0]));
    r.c1 = add(add(mont_mul(q0, k.a0[1]), mont_mul(q1, k.a1g2[1])), mont_mul(y, k.a2[1]));
    return r;
}
// one value per lane: N < 16, or buffers that are not 16-byte aligned.  A workgroup spans several proofs when N < 256: b is per lane.
__global__ __launch_bounds__(256) void compose_ext_batch_kernel(ComposeArgs a, const BatchChal* __restrict__ chal, const BatchChalExt* __restrict__ xchal,
                                                                size_t total) {
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= total) return;
    const size_t b = pos >> a.logN, i = pos & (((size_t)1 << a.logN) - 1);
    const ComposeExtConsts k = compose_ext_batch_consts(chal, xchal, b);
    const ComposeRaw r = compose_fetch(a, a.f + (b << a.logN), i);
    const uint32_t x = mont_mul(mont_mul(r.x_hi, r.x_lo), a.w_mont);
    const Ext v = compose_ext_batch_eval(a, k, r.f0, r.f1, r.f2, r.inv0, r.inv2, x, r.zz);
    a.cp[pos] = v.c0;
    a.cp[total + pos] = v.c1;
}
// compose_ext_kernel4 over the batch: four consecutive values of ONE proof per lane (N >= 16, so a group of four never straddles two
// proofs and the taps wrap inside the proof's own f), 16-byte loads, one 16-byte store per plane.
__global__ __launch_bounds__(256) void compose_ext_batch_kernel4(ComposeArgs a, const BatchChal* __restrict__ chal, const BatchChalExt* __restrict__ xchal,
                                                                 size_t total) {
    const size_t N = (size_t)1 << a.logN;
    const uint32_t B = 1u << a.log_b;
    const size_t pos = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (pos >= total) return;
    const size_t b = pos >> a.logN, i = pos & (N - 1);
    const ComposeExtConsts kc = compose_ext_batch_consts(chal, xchal, b);
    const uint4* fv = reinterpret_cast<const uint4*>(a.f + (b << a.logN));
    const uint4* iv = reinterpret_cast<const uint4*>(a.inv_xm1);
    uint32_t f0[4], f1[4], f2[4], inv0[4], inv2[4], zz[4];
    const uint4 v0 = fv[i >> 2], w0 = iv[i >> 2];
    f0[0] = v0.x; f0[1] = v0.y; f0[2] = v0.z; f0[3] = v0.w;
    inv0[0] = w0.x; inv0[1] = w0.y; inv0[2] = w0.z; inv0[3] = w0.w;
    if (B >= 4) {
        const uint4 v1 = fv[((i + B) & (N - 1)) >> 2], v2 = fv[((i + 2 * (size_t)B) & (N - 1)) >> 2], w2 = iv[((i + 2 * (size_t)B) & (N - 1)) >> 2];
        f1[0] = v1.x; f1[1] = v1.y; f1[2] = v1.z; f1[3] = v1.w;
        f2[0] = v2.x; f2[1] = v2.y; f2[2] = v2.z; f2[3] = v2.w;
        inv2[0] = w2.x; inv2[1] = w2.y; inv2[2] = w2.z; inv2[3] = w2.w;
        const uint32_t z0 = (uint32_t)i & (B - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) zz[k] = a.zz[z0 + k];
    } else {
        const uint4 v1 = fv[((i + 4) & (N - 1)) >> 2], w1 = iv[((i + 4) & (N - 1)) >> 2];
        const uint32_t fw[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        const uint32_t iw[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f1[k] = B == 1 ? fw[k + 1] : fw[k + 2];
            f2[k] = B == 1 ? fw[k + 2] : fw[k + 4];
            inv2[k] = B == 1 ? iw[k + 2] : iw[k + 4];
            zz[k] = B == 1 ? a.zz[0] : a.zz[k & 1];
        }
    }
    uint32_t x = mont_mul(pow_lookup(a.htab, (uint32_t)i), a.w_mont);
    const uint32_t h = pow_lookup(a.htab, 1u);
    Ext r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r[k] = compose_ext_batch_eval(a, kc, f0[k], f1[k], f2[k], inv0[k], inv2[k], x, zz[k]);
        if (k < 3) x = mont_mul(x, h);
    }
    reinterpret_cast<uint4*>(a.cp)[pos >> 2] = make_uint4(r[0].c0, r[1].c0, r[2].c0, r[3].c0);
    reinterpret_cast<uint4*>(a.cp)[(total + pos) >> 2] = make_uint4(r[0].c1, r[1].c1, r[2].c1, r[3].c1);
}
hipError_t launch_compose_ext_batch(const ComposeBatchArgs& a, const BatchChalExt* xchal, uint32_t batch, hipStream_t s, Profiler* prof) {
    if (!a.chal || !xchal || batch < 1 || ((uint64_t)batch << a.a.logN) > ((uint64_t)1 << 32)) return hipErrorInvalidValue;
    const size_t total = (size_t)batch << a.a.logN;
    ScopedKernelTimer tm(prof, K_COMPOSE, 12.0 * (double)total, s);   // read f once, write two planes
    const bool aligned = ((reinterpret_cast<uintptr_t>(a.a.f) | reinterpret_cast<uintptr_t>(a.a.inv_xm1) | reinterpret_cast<uintptr_t>(a.a.cp)) & 15u) == 0;
    if (a.a.logN >= 4 && aligned) hipLaunchKernelGGL(compose_ext_batch_kernel4, dim3((uint32_t)((total / 4 + 255) / 256)), dim3(256), 0, s, a.a, a.chal, xchal, total);
    else hipLaunchKernelGGL(compose_ext_batch_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, a.a, a.chal, xchal, total);
    return hipGetLastError();
}

// CP = sum_b cp_b (mod P) of a proof-major batch, for the shared proof (transcript.hpp "lb"): a.cp[i], i < N, from a.f = [batch][N].
// The denominators of the three constraints, x and the vanishing product depend on i alone, so they are taken once per i and the sum
// runs over the numerators:
//   CP(i) = inv0 S0 + inv2 S1 + y S2,  S0 = sum_b alpha0_b (f_b[i] - first_b),  S1 = sum_b alpha1g2_b (f_b[i] - last_b),
//   S2 = sum_b alpha2_b (f_b[i+2B] - f_b[i+B]^2 - f_b[i]^2)
// with compose_eval's Montgomery scales: S0 and S1 are canonical sums, S2 carries R^-1 and y = V / (x^n - 1) R^2.  Per statement that is
// three loads and six multiplications per value; chal[b] is read wave-uniformly (b is the loop counter).
__device__ __forceinline__ void compose_sum_term(uint32_t f0, uint32_t f1, uint32_t f2, uint32_t first, uint32_t last, uint32_t al0, uint32_t al1g2,
                                                 uint32_t al2, uint32_t& s0, uint32_t& s1, uint32_t& s2) {
    s0 = add(s0, mont_mul(sub(f0, first), al0));
    s1 = add(s1, mont_mul(sub(f0, last), al1g2));
    const uint32_t num = sub(sub(mont_mul(f2, 1u), mont_mul(f1, f1)), mont_mul(f0, f0));
    s2 = add(s2, mont_mul(num, al2));
}
__device__ __forceinline__ uint32_t compose_sum_finish(const ComposeArgs& a, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t inv0, uint32_t inv2, uint32_t x,
                                                       uint32_t zz) {
    const uint32_t v3 = mont_mul(mont_mul(sub(x, a.gm3_mont), sub(x, a.gm2_mont)), sub(x, a.gm1_mont));
    return add(add(mont_mul(s0, inv0), mont_mul(s1, inv2)), mont_mul(s2, mont_mul(v3, zz)));
}
// vec: four consecutive i per thread with 16-byte accesses and compose_kernel4's taps (whole vectors for B >= 4, windows of the vectors
// at i and i + 4 for B = 1, 2); the next statement's vectors are loaded before the arithmetic of the current one.  !vec (logN < 4, or
// unaligned pointers): one i per thread.
__global__ __launch_bounds__(256) void compose_sum_batch_kernel(ComposeArgs a, const BatchChal* __restrict__ chal, uint32_t batch, uint32_t vec) {
    const size_t N = (size_t)1 << a.logN;
    const uint32_t B = 1u << a.log_b;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!vec) {
        if (t >= N) return;
        const size_t i1 = (t + B) & (N - 1), i2 = (t + 2 * (size_t)B) & (N - 1);
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        for (uint32_t b = 0; b < batch; ++b) {
            const uint32_t* f = a.f + ((size_t)b << a.logN);
            compose_sum_term(f[t], f[i1], f[i2], chal[b].first, chal[b].last, chal[b].alpha0_mont, chal[b].alpha1g2_mont, chal[b].alpha2_mont, s0, s1, s2);
        }
        const uint32_t x = mont_mul(pow_lookup(a.htab, (uint32_t)t), a.w_mont);
        a.cp[t] = compose_sum_finish(a, s0, s1, s2, a.inv_xm1[t], a.inv_xm1[i2], x, a.zz[t & (B - 1)]);
        return;
    }
    const size_t i = t * 4;
    if (i >= N) return;
    const uint4* fv = reinterpret_cast<const uint4*>(a.f);
    const uint4* iv = reinterpret_cast<const uint4*>(a.inv_xm1);
    const bool wide = B >= 4;
    // q2: the third vector of a statement (B < 4: the window needs two, and the third is the second again)
    const size_t q0 = i >> 2, q1 = ((i + (wide ? B : 4u)) & (N - 1)) >> 2, q2 = wide ? ((i + 2 * (size_t)B) & (N - 1)) >> 2 : q1, stride = N >> 2;
    uint32_t inv0[4], inv2[4], zz[4];
    {
        const uint4 w0 = iv[q0];
        inv0[0] = w0.x; inv0[1] = w0.y; inv0[2] = w0.z; inv0[3] = w0.w;
        if (wide) {
            const uint4 w2 = iv[q2];   // wide: q2 is the vector at i + 2B
            inv2[0] = w2.x; inv2[1] = w2.y; inv2[2] = w2.z; inv2[3] = w2.w;
            const uint32_t z0 = (uint32_t)i & (B - 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) zz[k] = a.zz[z0 + k];
        } else {
            const uint4 w1 = iv[q1];
            const uint32_t iw[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                inv2[k] = B == 1 ? iw[k + 2] : iw[k + 4];
                zz[k] = B == 1 ? a.zz[0] : a.zz[k & 1];
            }
        }
    }
    uint32_t s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    uint4 c0 = fv[q0], c1 = fv[q1], c2 = fv[q2];
    for (uint32_t b = 0; b < batch; ++b) {
        uint4 n0 = c0, n1 = c1, n2 = c2;
        if (b + 1 < batch) {                                  // the next statement's loads, in flight across this one's arithmetic
            const size_t nx = (size_t)(b + 1) * stride;
            n0 = fv[nx + q0]; n1 = fv[nx + q1]; n2 = fv[nx + q2];
        }
        const uint32_t first = chal[b].first, last = chal[b].last, al0 = chal[b].alpha0_mont, al1g2 = chal[b].alpha1g2_mont, al2 = chal[b].alpha2_mont;
        const uint32_t fw[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const uint32_t f2w[4] = {c2.x, c2.y, c2.z, c2.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t f1 = wide ? fw[4 + k] : B == 1 ? fw[k + 1] : fw[k + 2];
            const uint32_t f2 = wide ? f2w[k] : B == 1 ? fw[k + 2] : fw[k + 4];
            compose_sum_term(fw[k], f1, f2, first, last, al0, al1g2, al2, s0[k], s1[k], s2[k]);
        }
        c0 = n0; c1 = n1; c2 = n2;
    }
    uint32_t x = mont_mul(pow_lookup(a.htab, (uint32_t)i), a.w_mont);
    const uint32_t h = pow_lookup(a.htab, 1u);
    uint32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r[k] = compose_sum_finish(a, s0[k], s1[k], s2[k], inv0[k], inv2[k], x, zz[k]);
        if (k < 3) x = mont_mul(x, h);
    }
    reinterpret_cast<uint4*>(a.cp)[i >> 2] = make_uint4(r[0], r[1], r[2], r[3]);
}
hipError_t launch_compose_sum_batch(const ComposeBatchArgs& a, uint32_t log_batch, hipStream_t s, Profiler* prof) {
    if (!a.chal || a.a.logN + log_batch > 32) return hipErrorInvalidValue;
    const size_t N = (size_t)1 << a.a.logN;
    const uint32_t batch = 1u << log_batch;
    ScopedKernelTimer tm(prof, K_COMPOSE, 4.0 * (double)N * (double)batch + 4.0 * (double)N, s);   // read every f once, write CP once
    const bool aligned = ((reinterpret_cast<uintptr_t>(a.a.f) | reinterpret_cast<uintptr_t>(a.a.inv_xm1) | reinterpret_cast<uintptr_t>(a.a.cp)) & 15u) == 0;
    const uint32_t vec = a.a.logN >= 4 && aligned;
    hipLaunchKernelGGL(compose_sum_batch_kernel, dim3((uint32_t)(((vec ? N / 4 : N) + 255) / 256)), dim3(256), 0, s, a.a, a.chal, batch, vec);
    return hipGetLastError();
}

// ===========================================================================
// FRI fold
// ===========================================================================
// next[i] = (e[i] + e[i+m/2])/2 + beta (e[i] - e[i+m/2]) / (2 x_i),  x_i = (w h^i)^(2^r)
// (identity pinned by fri_test, polynomial.rs:418-425, and used at proof.rs:110-113).
struct FoldRaw { uint32_t u, v, x_hi, x_lo; };
__device__ __forceinline__ FoldRaw fold_fetch(const FoldArgs& a, size_t i) {
    const size_t half = (size_t)1 << (a.log_m - 1);
    const uint32_t e = (uint32_t)(i << a.round);                    // h^(-2^r i), i 2^r < N/2
    FoldRaw r;
    r.u = a.in[i]; r.v = a.in[i + half];
    r.x_hi = a.hinv.hi[e >> a.hinv.lo_bits]; r.x_lo = a.hinv.lo[e & ((1u << a.hinv.lo_bits) - 1u)];
    return r;
}
__device__ __forceinline__ uint32_t fold_finish(const FoldArgs& a, const FoldRaw& r) {
    uint32_t xinv = mont_mul(r.x_hi, r.x_lo);
    uint32_t s = mont_mul(add(r.u, r.v), a.inv2_mont);
    uint32_t d = mont_mul(mont_mul(sub(r.u, r.v), xinv), a.c_mont);
    return add(s, d);
}
__device__ __forceinline__ uint32_t fold_at(const FoldArgs& a, size_t i) { return fold_finish(a, fold_fetch(a, i)); }

__global__ __launch_bounds__(256) void fri_fold_kernel(FoldArgs a) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ((size_t)1 << (a.log_m - 1))) return;
    a.out[i] = fold_at(a, i);
}

// four consecutive outputs per thread, 16-byte accesses; x^-1 advances by h^(-2^r)
__global__ __launch_bounds__(256) void fri_fold_kernel4(FoldArgs a) {
    const size_t half = (size_t)1 << (a.log_m - 1);
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= half) return;
    const uint4 u = reinterpret_cast<const uint4*>(a.in)[i >> 2], v = reinterpret_cast<const uint4*>(a.in)[(i + half) >> 2];
    const uint32_t uu[4] = {u.x, u.y, u.z, u.w}, vv[4] = {v.x, v.y, v.z, v.w};
    uint32_t xinv = pow_lookup(a.hinv, (uint32_t)(i << a.round));
    const uint32_t step = pow_lookup(a.hinv, 1u << a.round);
    uint32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t sm = mont_mul(add(uu[k], vv[k]), a.inv2_mont);
        const uint32_t d = mont_mul(mont_mul(sub(uu[k], vv[k]), xinv), a.c_mont);
        r[k] = add(sm, d);
        if (k < 3) xinv = mont_mul(xinv, step);
    }
    reinterpret_cast<uint4*>(a.out)[i >> 2] = make_uint4(r[0], r[1], r[2], r[3]);
}

hipError_t launch_fri_fold(const FoldArgs& a, hipStream_t s, Profiler* prof) {
    size_t half = (size_t)1 << (a.log_m - 1);
    ScopedKernelTimer tm(prof, K_FOLD, 12.0 * (double)half, s);   // read m words, write m/2
    const bool aligned = ((reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(a.out)) & 15u) == 0;
    if (half >= 4 && aligned) {
        uint32_t blocks = (uint32_t)((half / 4 + 255) / 256);
        hipLaunchKernelGGL(fri_fold_kernel4, dim3(blocks), dim3(256), 0, s, a);
    } else {
        uint32_t blocks = (uint32_t)((half + 255) / 256);
        hipLaunchKernelGGL(fri_fold_kernel, dim3(blocks), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

// ---- fold by 2^STEPS in one pass (FoldMultiArgs) ---------------------------------------------------------------
// v[t] = in[i + t m / S].  Step k: v[t] <- (v[t] + v[t + cnt]) + (v[t] - v[t + cnt]) * xinv^(2^k) * c[k][t], cnt = S >> (k+1);
// xinv = h^(-2^r i) by one table look-up, squared between the steps; out[i] = v[0] * 2^-STEPS.
template <int STEPS>
__device__ __forceinline__ uint32_t fold_multi_core(const uint32_t (&c)[7], uint32_t scale_mont, uint32_t (&v)[1 << STEPS], uint32_t xinv) {
    constexpr int S = 1 << STEPS;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const int cnt = S >> (k + 1);
#pragma unroll
        for (int t = 0; t < cnt; ++t) {
            const uint32_t u = v[t], w = v[t + cnt];
            v[t] = add(add(u, w), mont_mul(sub(u, w), mont_mul(xinv, c[S - (S >> k) + t])));
        }
        if (k + 1 < STEPS) xinv = mont_mul(xinv, xinv);
    }
    return mont_mul(v[0], scale_mont);
}
template <int STEPS>
__device__ __forceinline__ uint32_t fold_multi_one(const FoldMultiArgs& a, uint32_t (&v)[1 << STEPS], uint32_t xinv) {
    return fold_multi_core<STEPS>(a.c_mont, a.scale_mont, v, xinv);
}

template <int STEPS>
__global__ __launch_bounds__(256) void fri_fold_multi_kernel1(FoldMultiArgs a) {
    constexpr int S = 1 << STEPS;
    const size_t q = (size_t)1 << (a.log_m - STEPS);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q) return;
    uint32_t v[S];
#pragma unroll
    for (int t = 0; t < S; ++t) v[t] = a.in[i + t * q];
    a.out[i] = fold_multi_one<STEPS>(a, v, pow_lookup(a.hinv, (uint32_t)(i << a.round)));
}

// four consecutive outputs per thread: S coalesced 16-byte loads, one 16-byte store; x^-1 advances by h^(-2^r)
template <int STEPS>
__global__ __launch_bounds__(256) void fri_fold_multi_kernel(FoldMultiArgs a) {
    constexpr int S = 1 << STEPS;
    const size_t q = (size_t)1 << (a.log_m - STEPS);
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= q) return;
    uint4 ld[S];
#pragma unroll
    for (int t = 0; t < S; ++t) ld[t] = reinterpret_cast<const uint4*>(a.in)[(i + t * q) >> 2];
    uint32_t xinv = pow_lookup(a.hinv, (uint32_t)(i << a.round));
    const uint32_t step = pow_lookup(a.hinv, 1u << a.round);
    uint32_t r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t v[S];
#pragma unroll
        for (int t = 0; t < S; ++t) v[t] = e == 0 ? ld[t].x : e == 1 ? ld[t].y : e == 2 ? ld[t].z : ld[t].w;
        r[e] = fold_multi_one<STEPS>(a, v, xinv);
        if (e < 3) xinv = mont_mul(xinv, step);
    }
    reinterpret_cast<uint4*>(a.out)[i >> 2] = make_uint4(r[0], r[1], r[2], r[3]);
}

template <int STEPS>
static void fold_multi_launch(const FoldMultiArgs& a, size_t q, bool wide, hipStream_t s) {
    if (wide) hipLaunchKernelGGL(fri_fold_multi_kernel<STEPS>, dim3((uint32_t)((q / 4 + 255) / 256)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(fri_fold_multi_kernel1<STEPS>, dim3((uint32_t)((q + 255) / 256)), dim3(256), 0, s, a);
}
hipError_t launch_fri_fold_multi(const FoldMultiArgs& a, hipStream_t s, Profiler* prof) {
    if (a.steps < 1 || a.steps > 3 || a.log_m < a.steps) return hipErrorInvalidValue;
    const size_t m = (size_t)1 << a.log_m, q = m >> a.steps;
    ScopedKernelTimer tm(prof, K_FOLD, 4.0 * (double)(m + q), s);   // read m words, write m / S
    const bool wide = q >= 4 && ((reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(a.out)) & 15u) == 0;
    if (a.steps == 1) fold_multi_launch<1>(a, q, wide, s);
    else if (a.steps == 2) fold_multi_launch<2>(a, q, wide, s);
    else fold_multi_launch<3>(a, q, wide, s);
    return hipGetLastError();
}

// ---- the same butterfly over E (FoldMultiExtArgs) -------------------------------------------------------------------
// Values and challenge constants in E, the point in the base field: (u - w) is scaled by xinv^(2^k) (two multiplications), then taken
// times the constant of E (four and two additions, ext_mul_const).  With a challenge (beta0, 0) every constant has c1 = 0 and each
// plane is fold_multi_core of that plane.
template <int STEPS>
__device__ __forceinline__ Ext fold_multi_ext_core(const ExtConst (&c)[7], uint32_t scale_mont, Ext (&v)[1 << STEPS], uint32_t xinv) {
    constexpr int S = 1 << STEPS;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const int cnt = S >> (k + 1);
#pragma unroll
        for (int t = 0; t < cnt; ++t) {
            const Ext u = v[t], w = v[t + cnt];
            v[t] = ext_add(ext_add(u, w), ext_mul_const(ext_scale(ext_sub(u, w), xinv), c[S - (S >> k) + t]));
        }
        if (k + 1 < STEPS) xinv = mont_mul(xinv, xinv);
    }
    return ext_scale(v[0], scale_mont);
}

template <int STEPS>
__global__ __launch_bounds__(256) void fri_fold_multi_ext_kernel1(FoldMultiExtArgs a) {
    constexpr int S = 1 << STEPS;
    const size_t m = (size_t)1 << a.log_m, q = m >> STEPS;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q) return;
    Ext v[S];
#pragma unroll
    for (int t = 0; t < S; ++t) v[t] = Ext{a.in[i + t * q], a.in[m + i + t * q]};
    const Ext r = fold_multi_ext_core<STEPS>(a.c, a.scale_mont, v, pow_lookup(a.hinv, (uint32_t)(i << a.round)));
    a.out[i] = r.c0;
    a.out[q + i] = r.c1;
}

// four consecutive outputs per thread: S coalesced 16-byte loads and one 16-byte store per plane; x^-1 advances by h^(-2^r).  The
// STEPS = 3 instance holds its sixteen loads in registers (81 VGPRs as built, no scratch: DESIGN.md 7j), so every instance takes four.
template <int STEPS>
__global__ __launch_bounds__(256) void fri_fold_multi_ext_kernel(FoldMultiExtArgs a) {
    constexpr int S = 1 << STEPS;
    const size_t m = (size_t)1 << a.log_m, q = m >> STEPS;
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= q) return;
    uint4 l0[S], l1[S];
#pragma unroll
    for (int t = 0; t < S; ++t) {
        l0[t] = reinterpret_cast<const uint4*>(a.in)[(i + t * q) >> 2];
        l1[t] = reinterpret_cast<const uint4*>(a.in)[(m + i + t * q) >> 2];
    }
    uint32_t xinv = pow_lookup(a.hinv, (uint32_t)(i << a.round));
    const uint32_t step = pow_lookup(a.hinv, 1u << a.round);
    Ext r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        Ext v[S];
#pragma unroll
        for (int t = 0; t < S; ++t)
            v[t] = e == 0 ? Ext{l0[t].x, l1[t].x} : e == 1 ? Ext{l0[t].y, l1[t].y} : e == 2 ? Ext{l0[t].z, l1[t].z} : Ext{l0[t].w, l1[t].w};
        r[e] = fold_multi_ext_core<STEPS>(a.c, a.scale_mont, v, xinv);
        if (e < 3) xinv = mont_mul(xinv, step);
    }
    reinterpret_cast<uint4*>(a.out)[i >> 2] = make_uint4(r[0].c0, r[1].c0, r[2].c0, r[3].c0);
    reinterpret_cast<uint4*>(a.out)[(q + i) >> 2] = make_uint4(r[0].c1, r[1].c1, r[2].c1, r[3].c1);
}

template <int STEPS>
static void fold_multi_ext_launch(const FoldMultiExtArgs& a, size_t q, bool wide, hipStream_t s) {
    if (wide) hipLaunchKernelGGL(fri_fold_multi_ext_kernel<STEPS>, dim3((uint32_t)((q / 4 + 255) / 256)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(fri_fold_multi_ext_kernel1<STEPS>, dim3((uint32_t)((q + 255) / 256)), dim3(256), 0, s, a);
}
hipError_t launch_fri_fold_multi_ext(const FoldMultiExtArgs& a, hipStream_t s, Profiler* prof) {
    if (a.steps < 1 || a.steps > 3 || a.log_m < a.steps) return hipErrorInvalidValue;
    const size_t m = (size_t)1 << a.log_m, q = m >> a.steps;
    ScopedKernelTimer tm(prof, K_FOLD, 8.0 * (double)(m + q), s);   // read two planes of m words, write two of m / S
    const bool wide = q >= 4 && ((reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(a.out)) & 15u) == 0;
    if (a.steps == 1) fold_multi_ext_launch<1>(a, q, wide, s);
    else if (a.steps == 2) fold_multi_ext_launch<2>(a, q, wide, s);
    else fold_multi_ext_launch<3>(a, q, wide, s);
    return hipGetLastError();
}

// ---- the same over a proof-major batch (FoldMultiBatchArgs): in = [batch][m], out = [batch][m / S], proof b with its own challenge ----
// One lane per proof turns the raw challenge into the proof's row of constants: cb[8 b + j] = beta_b^(2^k) * a.c_mont[j] for the
// S - 1 slots j = S - (S >> k) + t the butterfly reads (a.c_mont holds the root-of-unity part only), the rest of the row 0.
template <int STEPS>
__global__ __launch_bounds__(256) void fri_fold_multi_batch_prep_kernel(FoldMultiBatchArgs p) {
    constexpr int S = 1 << STEPS;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.batch) return;
    uint32_t bk = mont_mul(p.beta_raw[(size_t)b * p.beta_stride], R2_MONT);   // any u32 -> beta mod P, Montgomery form (field.rs:20-24)
    uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
#pragma unroll
        for (int t = 0; t < (S >> (k + 1)); ++t) c[S - (S >> k) + t] = mont_mul(bk, p.a.c_mont[S - (S >> k) + t]);
        if (k + 1 < STEPS) bk = mont_mul(bk, bk);
    }
    uint32_t* row = p.cb + (size_t)b * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) row[j] = c[j];
}
template <int STEPS>
__device__ __forceinline__ void fold_multi_batch_consts(const FoldMultiBatchArgs& p, size_t b, uint32_t (&c)[7]) {
    constexpr int S = 1 << STEPS;
    const uint32_t* row = p.cb + b * 8;
#pragma unroll
    for (int j = 0; j < 7; ++j) c[j] = j < S - 1 ? row[j] : 0u;
}

// one output per lane: per-proof outputs of fewer than 4 values, or buffers that are not 16-byte aligned
template <int STEPS>
__global__ __launch_bounds__(256) void fri_fold_multi_batch_kernel1(FoldMultiBatchArgs p) {
    constexpr int S = 1 << STEPS;
    const uint32_t log_q = p.a.log_m - STEPS;
    const size_t q = (size_t)1 << log_q;
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= ((size_t)p.batch << log_q)) return;
    const size_t b = pos >> log_q, i = pos & (q - 1);
    const uint32_t* in = p.a.in + (b << p.a.log_m);
    uint32_t v[S];
#pragma unroll
    for (int t = 0; t < S; ++t) v[t] = in[i + t * q];
    uint32_t c[7];
    fold_multi_batch_consts<STEPS>(p, b, c);
    p.a.out[pos] = fold_multi_core<STEPS>(c, p.a.scale_mont, v, pow_lookup(p.a.hinv, (uint32_t)(i << p.a.round)));
}

// four consecutive outputs of one proof per lane (m / S >= 4, so a group of four never straddles two proofs): S coalesced 16-byte
// loads, one 16-byte store, one table look-up advanced by h^(-2^r)
template <int STEPS>
__global__ __launch_bounds__(256) void fri_fold_multi_batch_kernel(FoldMultiBatchArgs p) {
    constexpr int S = 1 << STEPS;
    const uint32_t log_q = p.a.log_m - STEPS;
    const size_t q = (size_t)1 << log_q;
    const size_t pos = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (pos >= ((size_t)p.batch << log_q)) return;
    const size_t b = pos >> log_q, i = pos & (q - 1);
    const uint32_t* in = p.a.in + (b << p.a.log_m);
    uint4 ld[S];
#pragma unroll
    for (int t = 0; t < S; ++t) ld[t] = reinterpret_cast<const uint4*>(in)[(i + t * q) >> 2];
    uint32_t c[7];
    fold_multi_batch_consts<STEPS>(p, b, c);
    uint32_t xinv = pow_lookup(p.a.hinv, (uint32_t)(i << p.a.round));
    const uint32_t step = pow_lookup(p.a.hinv, 1u << p.a.round);
    uint32_t r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t v[S];
#pragma unroll
        for (int t = 0; t < S; ++t) v[t] = e == 0 ? ld[t].x : e == 1 ? ld[t].y : e == 2 ? ld[t].z : ld[t].w;
        r[e] = fold_multi_core<STEPS>(c, p.a.scale_mont, v, xinv);
        if (e < 3) xinv = mont_mul(xinv, step);
    }
    reinterpret_cast<uint4*>(p.a.out)[pos >> 2] = make_uint4(r[0], r[1], r[2], r[3]);
}

template <int STEPS>
static void fold_multi_batch_launch(const FoldMultiBatchArgs& p, size_t total, bool wide, hipStream_t s) {
    hipLaunchKernelGGL(fri_fold_multi_batch_prep_kernel<STEPS>, dim3((p.batch + 255) / 256), dim3(256), 0, s, p);
    if (wide) hipLaunchKernelGGL(fri_fold_multi_batch_kernel<STEPS>, dim3((uint32_t)((total / 4 + 255) / 256)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(fri_fold_multi_batch_kernel1<STEPS>, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, p);
}
hipError_t launch_fri_fold_multi_batch(const FoldMultiBatchArgs& p, hipStream_t s, Profiler* prof) {
    const FoldMultiArgs& a = p.a;
    if (a.steps < 1 || a.steps > 3 || a.log_m < a.steps || a.log_m > 32 || p.batch < 1 || !p.beta_raw || !p.cb) return hipErrorInvalidValue;
    const size_t m = (size_t)1 << a.log_m, q = m >> a.steps, total = (size_t)p.batch * q;
    if ((size_t)p.batch * m > ((size_t)1 << 32)) return hipErrorInvalidValue;
    ScopedKernelTimer tm(prof, K_FOLD, 4.0 * (double)p.batch * (double)(m + q), s);   // read batch * m words, write batch * m / S
    const bool wide = q >= 4 && ((reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(a.out)) & 15u) == 0;
    if (a.steps == 1) fold_multi_batch_launch<1>(p, total, wide, s);
    else if (a.steps == 2) fold_multi_batch_launch<2>(p, total, wide, s);
    else fold_multi_batch_launch<3>(p, total, wide, s);
    return hipGetLastError();
}

// ---- the butterfly over E for a proof-major batch (FoldMultiExtBatchArgs) ---------------------------------------------
// One lane per proof reduces the raw (c0, c1) of its challenge, squares it in E between the steps and writes its row of cb: ExtConst j
// at words 3 j .. 3 j + 2 = beta^(2^k) * a.c_mont[j] (c0, c1, 5 c1; Montgomery), j = S - (S >> k) + t the slots the butterfly reads,
// the rest of the kFoldExtRow words 0.  The arithmetic stays in Montgomery form; the residues are fold_multi_ext_args' (domain.hip).
constexpr uint32_t FIVE_MONT = (uint32_t)(((uint64_t)EXT_NONRESIDUE * R1) % P);
template <int STEPS>
__global__ __launch_bounds__(256) void fri_fold_multi_ext_batch_prep_kernel(FoldMultiExtBatchArgs p) {
    constexpr int S = 1 << STEPS;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.batch) return;
    uint32_t b0 = mont_mul(p.beta0_raw[(size_t)b * p.stride0], R2_MONT);   // any u32 -> the residue mod P, Montgomery form (field.rs:20-24)
    uint32_t b1 = mont_mul(p.beta1_raw[(size_t)b * p.stride1], R2_MONT);
    uint32_t row[kFoldExtRow];
#pragma unroll
    for (uint32_t j = 0; j < kFoldExtRow; ++j) row[j] = 0u;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
#pragma unroll
        for (int t = 0; t < (S >> (k + 1)); ++t) {
            const int j = S - (S >> k) + t;
            const uint32_t c1 = mont_mul(b1, p.a.c_mont[j]);
            row[3 * j] = mont_mul(b0, p.a.c_mont[j]); row[3 * j + 1] = c1; row[3 * j + 2] = mont_mul(c1, FIVE_MONT);
        }
        if (k + 1 < STEPS) {                                               // (b0 + b1 u)^2 = b0^2 + 5 b1^2 + 2 b0 b1 u
            const uint32_t cross = mont_mul(b0, b1);
            b0 = add(mont_mul(b0, b0), mont_mul(mont_mul(b1, b1), FIVE_MONT));
            b1 = add(cross, cross);
        }
    }
    uint4* out = reinterpret_cast<uint4*>(p.cb + (size_t)b * kFoldExtRow);
#pragma unroll
    for (uint32_t j = 0; j < kFoldExtRow / 4; ++j) out[j] = make_uint4(row[4 * j], row[4 * j + 1], row[4 * j + 2], row[4 * j + 3]);
}
// Proof b's constants.  UNIFORM: every lane of the wave works on proof b (the caller made b wave-uniform), and the row was written by
// the launch before this one, so it is read through the constant address space -- scalar loads into SGPRs, no vector registers.
template <int STEPS, bool UNIFORM>
__device__ __forceinline__ void fold_multi_ext_batch_consts(const uint32_t* cb, size_t b, ExtConst (&c)[7]) {
    constexpr int S = 1 << STEPS;
    if constexpr (UNIFORM) {
        const __attribute__((address_space(4))) uint32_t* row = (const __attribute__((address_space(4))) uint32_t*)(cb + b * kFoldExtRow);
#pragma unroll
        for (int j = 0; j < 7; ++j) c[j] = j < S - 1 ? ExtConst{row[3 * j], row[3 * j + 1], row[3 * j + 2]} : ExtConst{0u, 0u, 0u};
    } else {
        const uint32_t* row = cb + b * kFoldExtRow;
#pragma unroll
        for (int j = 0; j < 7; ++j) c[j] = j < S - 1 ? ExtConst{row[3 * j], row[3 * j + 1], row[3 * j + 2]} : ExtConst{0u, 0u, 0u};
    }
}
template <int STEPS, bool UNIFORM>
__device__ __forceinline__ void fold_multi_ext_batch_one(const FoldMultiExtBatchArgs& p, size_t pos, size_t b, size_t total_in, size_t total_out) {
    constexpr int S = 1 << STEPS;
    const uint32_t log_q = p.a.log_m - STEPS;
    const size_t q = (size_t)1 << log_q, i = pos & (q - 1);
    const uint32_t* in = p.a.in + (b << p.a.log_m);
    Ext v[S];
#pragma unroll
    for (int t = 0; t < S; ++t) v[t] = Ext{in[i + t * q], in[total_in + i + t * q]};
    ExtConst c[7];
    fold_multi_ext_batch_consts<STEPS, UNIFORM>(p.cb, b, c);
    const Ext r = fold_multi_ext_core<STEPS>(c, p.a.scale_mont, v, pow_lookup(p.a.hinv, (uint32_t)(i << p.a.round)));
    p.a.out[pos] = r.c0;
    p.a.out[total_out + pos] = r.c1;
}
// one output per lane: per-proof outputs of fewer than 4 values, or planes that are not 16-byte aligned.  A wave's 64 positions lie in
// one proof when q >= 64 (a uniform test on a kernel argument).
template <int STEPS>
__global__ __launch_bounds__(256) void fri_fold_multi_ext_batch_kernel1(FoldMultiExtBatchArgs p) {
    const uint32_t log_q = p.a.log_m - STEPS;
    const size_t total_out = (size_t)p.batch << log_q, total_in = (size_t)p.batch << p.a.log_m;
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= total_out) return;
    const uint32_t b = (uint32_t)(pos >> log_q);
    if (log_q >= 6) fold_multi_ext_batch_one<STEPS, true>(p, pos, __builtin_amdgcn_readfirstlane(b), total_in, total_out);
    else fold_multi_ext_batch_one<STEPS, false>(p, pos, b, total_in, total_out);
}
template <int STEPS, bool UNIFORM>
__device__ __forceinline__ void fold_multi_ext_batch_four(const FoldMultiExtBatchArgs& p, size_t pos, size_t b, size_t total_in, size_t total_out) {
    constexpr int S = 1 << STEPS;
    const uint32_t log_q = p.a.log_m - STEPS;
    const size_t q = (size_t)1 << log_q, i = pos & (q - 1);
    const uint4* in = reinterpret_cast<const uint4*>(p.a.in + (b << p.a.log_m));
    uint4 l0[S], l1[S];
#pragma unroll
    for (int t = 0; t < S; ++t) {
        l0[t] = in[(i + t * q) >> 2];
        l1[t] = in[(total_in + i + t * q) >> 2];
    }
    ExtConst c[7];
    fold_multi_ext_batch_consts<STEPS, UNIFORM>(p.cb, b, c);
    uint32_t xinv = pow_lookup(p.a.hinv, (uint32_t)(i << p.a.round));
    const uint32_t step = pow_lookup(p.a.hinv, 1u << p.a.round);
    Ext r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        Ext v[S];
#pragma unroll
        for (int t = 0; t < S; ++t)
            v[t] = e == 0 ? Ext{l0[t].x, l1[t].x} : e == 1 ? Ext{l0[t].y, l1[t].y} : e == 2 ? Ext{l0[t].z, l1[t].z} : Ext{l0[t].w, l1[t].w};
        r[e] = fold_multi_ext_core<STEPS>(c, p.a.scale_mont, v, xinv);
        if (e < 3) xinv = mont_mul(xinv, step);
    }
    reinterpret_cast<uint4*>(p.a.out)[pos >> 2] = make_uint4(r[0].c0, r[1].c0, r[2].c0, r[3].c0);
    reinterpret_cast<uint4*>(p.a.out)[(total_out + pos) >> 2] = make_uint4(r[0].c1, r[1].c1, r[2].c1, r[3].c1);
}
// four consecutive outputs of one proof per lane (q >= 4, so a group of four never straddles two proofs): S coalesced 16-byte loads
// and one 16-byte store per plane.  A wave's 256 positions lie in one proof when q >= 256.
template <int STEPS>
__global__ __launch_bounds__(256) void fri_fold_multi_ext_batch_kernel(FoldMultiExtBatchArgs p) {
    const uint32_t log_q = p.a.log_m - STEPS;
    const size_t total_out = (size_t)p.batch << log_q, total_in = (size_t)p.batch << p.a.log_m;
    const size_t pos = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (pos >= total_out) return;
    const uint32_t b = (uint32_t)(pos >> log_q);
    if (log_q >= 8) fold_multi_ext_batch_four<STEPS, true>(p, pos, __builtin_amdgcn_readfirstlane(b), total_in, total_out);
    else fold_multi_ext_batch_four<STEPS, false>(p, pos, b, total_in, total_out);
}
template <int STEPS>
static void fold_multi_ext_batch_launch(const FoldMultiExtBatchArgs& p, size_t total, bool wide, hipStream_t s) {
    hipLaunchKernelGGL(fri_fold_multi_ext_batch_prep_kernel<STEPS>, dim3((p.batch + 255) / 256), dim3(256), 0, s, p);
    if (wide) hipLaunchKernelGGL(fri_fold_multi_ext_batch_kernel<STEPS>, dim3((uint32_t)((total / 4 + 255) / 256)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(fri_fold_multi_ext_batch_kernel1<STEPS>, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, p);
}
hipError_t launch_fri_fold_multi_ext_batch(const FoldMultiExtBatchArgs& p, hipStream_t s, Profiler* prof) {
    const FoldMultiArgs& a = p.a;
    if (a.steps < 1 || a.steps > 3 || a.log_m < a.steps || a.log_m > 32 || p.batch < 1 || !p.beta0_raw || !p.beta1_raw || !p.cb) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(p.cb) & 15u) != 0) return hipErrorInvalidValue;   // the rows are written 16 bytes at a time
    const size_t m = (size_t)1 << a.log_m, q = m >> a.steps, total = (size_t)p.batch * q;
    if ((size_t)p.batch * m > ((size_t)1 << 32)) return hipErrorInvalidValue;
    ScopedKernelTimer tm(prof, K_FOLD, 8.0 * (double)p.batch * (double)(m + q), s);   // read two planes of batch * m words, write two of batch * m / S
    // both planes of the input and of the output are 16-byte aligned when the first is and a plane is a multiple of four words
    const bool wide = q >= 4 && (total & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.in) | reinterpret_cast<uintptr_t>(a.out)) & 15u) == 0;
    if (a.steps == 1) fold_multi_ext_batch_launch<1>(p, total, wide, s);
    else if (a.steps == 2) fold_multi_ext_batch_launch<2>(p, total, wide, s);
    else fold_multi_ext_batch_launch<3>(p, total, wide, s);
    return hipGetLastError();
}

// ---- final polynomial of an early-stopped FRI (FinalPolyArgs) ------------------------------------------------------------------
// One workgroup holds the M <= 4096 values and the M / 2 twiddles w_M^-j in LDS (24 KiB), runs the log2 M radix-2 stages of the
// decimation-in-frequency inverse transform there (natural order in, bit-reversed out: position p ends as M q_bitrev(p), q(y) = p(s y))
// and writes c_k = q_k s^-k in natural order.  It sits on the proof's critical path once, so it is built for latency: up to 1024 lanes
// (two butterflies per lane and stage at M = 4096), the twiddles looked up once, nothing but LDS traffic between the barriers.  M may
// be smaller than the workgroup (M = 4: two butterflies); every barrier is outside the divergent loops.
constexpr uint32_t kFinalPolyThreads = 1024;
__global__ __launch_bounds__(kFinalPolyThreads) void fri_final_poly_kernel(FinalPolyArgs a) {
    __shared__ uint32_t x[1u << kFinalPolyMaxLog];
    __shared__ uint32_t tw[1u << (kFinalPolyMaxLog - 1)];
    __shared__ uint32_t high;
    const uint32_t M = 1u << a.log_m, pairs = M >> 1, tid = threadIdx.x, nt = blockDim.x;
    const uint32_t* in = a.in + (size_t)blockIdx.x * a.in_stride;
    uint32_t* out = a.out + (size_t)blockIdx.x * a.out_stride;
    if (tid == 0) high = 0;
    for (uint32_t i = tid; i < M; i += nt) x[i] = in[i];
    for (uint32_t j = tid; j < pairs; j += nt) tw[j] = pow_lookup(a.hinv, j << (a.L - a.log_m));
    __syncthreads();
    for (uint32_t lh = a.log_m; lh-- > 0; ) {                  // blocks of 2 * half values, twiddle w_(2 half)^-j = tw[j M / (2 half)]
        const uint32_t half = 1u << lh, tsh = a.log_m - 1 - lh;
        for (uint32_t b = tid; b < pairs; b += nt) {
            const uint32_t j = b & (half - 1), i0 = ((b - j) << 1) + j;
            const uint32_t u = x[i0], v = x[i0 + half];
            x[i0] = add(u, v);
            x[i0 + half] = mont_mul(sub(u, v), tw[j << tsh]);
        }
        __syncthreads();
    }
    uint32_t cnt = 0;
    for (uint32_t k = tid; k < M; k += nt) {
        uint32_t r = a.minv_mont, sp = a.sinv_mont;            // M^-1 s^-k by the bits of k (at most 12 steps)
        for (uint32_t e = k; e; e >>= 1) {
            if (e & 1) r = mont_mul(r, sp);
            sp = mont_mul(sp, sp);
        }
        const uint32_t c = mont_mul(x[__brev(k) >> (32 - a.log_m)], r);
        out[1 + k] = c;
        cnt += (k >= a.bound && c != 0) ? 1u : 0u;
    }
    if (cnt) atomicAdd(&high, cnt);                            // the one add: into LDS
    __syncthreads();
    if (tid == 0) out[0] = high;
}
hipError_t launch_fri_final_poly(const FinalPolyArgs& a, hipStream_t s, Profiler* prof) {
    if (a.log_m < 1 || a.log_m > kFinalPolyMaxLog || a.log_m > a.L || a.polys < 1 || !a.in || !a.out) return hipErrorInvalidValue;
    const uint32_t M = 1u << a.log_m;
    if (a.polys > 1 && (a.in_stride < M || a.out_stride < (size_t)M + 1)) return hipErrorInvalidValue;
    ScopedKernelTimer tm(prof, K_FOLD, 4.0 * (double)a.polys * (double)(2 * M + 1), s);   // read M words, write M + 1
    const uint32_t threads = M / 2 >= kFinalPolyThreads ? kFinalPolyThreads : (M / 2 <= 64 ? 64 : M / 2);
    hipLaunchKernelGGL(fri_final_poly_kernel, dim3(a.polys), dim3(threads), 0, s, a);
    return hipGetLastError();
}

// The same for a proof-major batch (launch_fri_final_poly_batch): one workgroup takes per = min(4096 / M, kFinalPolyBatchMaxPer)
// consecutive layers -- one contiguous run of per * M words -- into the same 16 KiB of LDS, builds the twiddle table once for all of
// them and runs every stage over the (layer, butterfly) pairs, so all lanes work at small M.  Only the count and the `bound` low
// coefficients of a layer are written ([polys][1 + bound]); the high ones are computed and counted per layer (LDS counters) and dropped.
// The last workgroup may hold fewer layers: `tot` bounds every loop.  The arithmetic per value is fri_final_poly_kernel's, in its order.
__global__ __launch_bounds__(kFinalPolyThreads) void fri_final_poly_batch_kernel(FinalPolyArgs a, uint32_t per) {
    __shared__ uint32_t x[1u << kFinalPolyMaxLog];
    __shared__ uint32_t tw[1u << (kFinalPolyMaxLog - 1)];
    __shared__ uint32_t high[kFinalPolyBatchMaxPer];
    const uint32_t M = 1u << a.log_m, pairs = M >> 1, tid = threadIdx.x, nt = blockDim.x;
    const uint32_t first = blockIdx.x * per;                   // < polys: the grid is ceil(polys / per)
    const uint32_t np = a.polys - first < per ? a.polys - first : per;
    const uint32_t tot = np << a.log_m;                        // <= 4096 values of this workgroup
    const uint32_t* in = a.in + ((size_t)first << a.log_m);
    uint32_t* out = a.out + (size_t)first * a.out_stride;
    for (uint32_t q = tid; q < np; q += nt) high[q] = 0;
    for (uint32_t i = tid; i < tot; i += nt) x[i] = in[i];
    for (uint32_t j = tid; j < pairs; j += nt) tw[j] = pow_lookup(a.hinv, j << (a.L - a.log_m));
    __syncthreads();
    for (uint32_t lh = a.log_m; lh-- > 0; ) {
        const uint32_t half = 1u << lh, tsh = a.log_m - 1 - lh;
        for (uint32_t t = tid; t < (tot >> 1); t += nt) {       // layer t / pairs, butterfly t % pairs
            const uint32_t b = t & (pairs - 1), j = b & (half - 1), i0 = ((t - b) << 1) + ((b - j) << 1) + j;
            const uint32_t u = x[i0], v = x[i0 + half];
            x[i0] = add(u, v);
            x[i0 + half] = mont_mul(sub(u, v), tw[j << tsh]);
        }
        __syncthreads();
    }
    for (uint32_t t = tid; t < tot; t += nt) {
        const uint32_t q = t >> a.log_m, k = t & (M - 1);
        uint32_t r = a.minv_mont, sp = a.sinv_mont;
        for (uint32_t e = k; e; e >>= 1) {
            if (e & 1) r = mont_mul(r, sp);
            sp = mont_mul(sp, sp);
        }
        const uint32_t c = mont_mul(x[(t - k) + (__brev(k) >> (32 - a.log_m))], r);
        if (k < a.bound) out[(size_t)q * a.out_stride + 1 + k] = c;
        else if (c != 0) atomicAdd(&high[q], 1u);              // into LDS; none for a trace that satisfies the constraints
    }
    __syncthreads();
    for (uint32_t q = tid; q < np; q += nt) out[(size_t)q * a.out_stride] = high[q];
}
hipError_t launch_fri_final_poly_batch(const FinalPolyArgs& a, hipStream_t s, Profiler* prof) {
    if (a.log_m < 1 || a.log_m > kFinalPolyMaxLog || a.log_m > a.L || a.polys < 1 || !a.in || !a.out) return hipErrorInvalidValue;
    const uint32_t M = 1u << a.log_m;
    if (a.bound < 1 || a.bound > M || a.in_stride != M || a.out_stride != (size_t)a.bound + 1) return hipErrorInvalidValue;
    uint32_t per = (1u << kFinalPolyMaxLog) >> a.log_m;
    if (per > kFinalPolyBatchMaxPer) per = kFinalPolyBatchMaxPer;
    ScopedKernelTimer tm(prof, K_FOLD, 4.0 * (double)a.polys * (double)(M + a.bound + 1), s);   // read M words, write bound + 1
    // one lane per butterfly of the fullest workgroup (the read-in and read-out loops then take two values per lane), in whole waves:
    // polys need not be a power of two (3 layers of M = 64 are 96 butterflies -> 128 lanes)
    const uint32_t most = (a.polys < per ? a.polys : per) << (a.log_m - 1);
    const uint32_t threads = most >= kFinalPolyThreads ? kFinalPolyThreads : ((most + 63u) & ~63u);
    hipLaunchKernelGGL(fri_final_poly_batch_kernel, dim3((a.polys + per - 1) / per), dim3(threads), 0, s, a, per);
    return hipGetLastError();
}

// ===========================================================================
// Merkle tree
// ===========================================================================
//
// Heap layout of merkle.rs:14-51: 2m-1 nodes, root 0, children of j at 2j+1, 2j+2,
// depth d occupies [2^d - 1, 2^(d+1) - 1), leaf i at m - 1 + i.
//
// SHA-256 is integer-VALU bound, so the design goal is 100 % lane utilisation with every
// HBM access a full line.  A wave owns 64 * 2^k consecutive inputs and walks them in groups of
// 64: group i is hashed by the 64 lanes (one coalesced 256 B / 2 KiB access), two sibling groups
// are paired through a 4 KiB LDS buffer into the 64 parents (lane j hashes children 2j, 2j+1), and
// so on up k levels like a binary counter -- every level keeps all 64 lanes busy and every
// digest is written once in a contiguous 2 KiB run.  All control flow is wave-uniform.  One launch lowers the tree by k levels; the last
// <= 2^11 nodes are finished by a single workgroup that keeps the level in LDS.

// Merkle hash selector (zk_hash_kind): 0 = SHA-256 (merkle.rs:1-2), 1 = field-native hash (fieldhash.hpp), 2 = BLAKE2s-256 (blake2s.hpp).
__constant__ FieldHashConsts g_fh_consts;       // Montgomery form: the 16-lane row form of the narrow levels (fieldhash_inner_row16)
__constant__ FieldHashConsts64 g_fh_consts64;   // canonical residues as doubles: every other field hash on the device (fieldhash_f64.hpp)

template <int HASH> struct Hasher;
template <> struct Hasher<0> {
    static __device__ __forceinline__ Digest leaf(uint32_t v) { return sha256_leaf(v); }
    static __device__ __forceinline__ Digest inner(const Digest& l, const Digest& r) { return sha256_inner(l, r); }
};
// The field hash runs in double precision on the device (round 5): the same function bit for bit, 0.74 of the time of the
// 32-bit Montgomery form in a dependent chain (tools/fh64_probe.hip, profiles/r05_fh64_probe.txt): an addition is one
// instruction instead of four when nothing has to be corrected.
template <> struct Hasher<1> {
    static __device__ __forceinline__ Digest leaf(uint32_t v) { return fieldhash_leaf64(v, g_fh_consts64); }
    static __device__ __forceinline__ Digest inner(const Digest& l, const Digest& r) { return fieldhash_inner64(l, r, g_fh_consts64); }
};
// BLAKE2s-256: one compression per leaf and per node, no schedule (blake2s.hpp; the byte order of a Digest is settled there).
template <> struct Hasher<2> {
    static __device__ __forceinline__ Digest leaf(uint32_t v) { return blake2s_leaf(v); }
    static __device__ __forceinline__ Digest inner(const Digest& l, const Digest& r) { return blake2s_inner(l, r); }
};

// Where the leaf values of a tree come from.  The prover fuses the elementwise producer of a layer
// into the leaf hashing of its commitment: the value is computed, written to the layer and hashed
// in one pass (no separate fold / compose launch, the layer is never re-read for hashing).
// A source is read in two steps so that the throughput kernel can have the memory reads of its NEXT group of 64 leaves
// in flight while it hashes the current one: fetch() only issues loads (what they return is `Raw`), finish() does the
// arithmetic and the store of the produced value.  load() = both, for the callers that take one value at a time.
struct PlainSrc {
    const uint32_t* vals;
    using Raw = uint32_t;
    __device__ __forceinline__ Raw fetch(size_t pos) const { return vals[pos]; }
    __device__ __forceinline__ uint32_t finish(const Raw& r, size_t) const { return r; }
    __device__ __forceinline__ uint32_t load(size_t pos) const { return vals[pos]; }
};
struct FoldSrc {       // FRI layer r+1 = fold(layer r, beta): prover.rs:198-211 + :214
    FoldArgs a;
    using Raw = FoldRaw;
    __device__ __forceinline__ void prepare() { if (a.dyn) a.c_mont = *a.dyn; }   // early launch: the challenge arrived after the enqueue
    __device__ __forceinline__ Raw fetch(size_t pos) const { return fold_fetch(a, pos); }
    __device__ __forceinline__ uint32_t finish(const Raw& r, size_t pos) const { uint32_t v = fold_finish(a, r); a.out[pos] = v; return v; }
    __device__ __forceinline__ uint32_t load(size_t pos) const { return finish(fetch(pos), pos); }
};
struct ComposeSrc {    // cp layer 0 from f_eval: prover.rs:101-173 + :176
    ComposeArgs a;
    using Raw = size_t;        // nothing fetched ahead: eight words in flight per lane cost more registers than the 2^24-leaf
                               // launch (four waves per SIMD hide the latency) gains -- measured 1 579 against 1 560 us
    __device__ __forceinline__ Raw fetch(size_t pos) const { return pos; }
    __device__ __forceinline__ uint32_t finish(const Raw& r, size_t) const { return load(r); }
    __device__ __forceinline__ uint32_t load(size_t pos) const { uint32_t v = compose_at(a, pos); a.cp[pos] = v; return v; }
};

struct ComposeBlockSrc {   // cp over this rank's block of a sharded proof, from the block of f it received (ComposeBlockArgs)
    ComposeBlockArgs b;
    using Raw = size_t;
    __device__ __forceinline__ uint32_t f_at(size_t t) const {
        const uint32_t gmask = (1u << b.lg) - 1u;
        if (t >> b.log_m) {                                     // the 2B positions after the block
            const size_t v = t - ((size_t)1 << b.log_m);
            return b.halo[(v & gmask) * b.halo_stride + (v >> b.lg)];
        }
        const uint32_t log_cl = b.lg + b.log_cnt;               // leaves per chunk of the exchange
        const size_t piece = ((t >> log_cl) << b.lg) | (t & gmask);
        return b.a.f[(piece << b.log_cnt) | ((t & (((size_t)1 << log_cl) - 1)) >> b.lg)];
    }
    __device__ __forceinline__ Raw fetch(size_t pos) const { return pos; }
    __device__ __forceinline__ uint32_t finish(const Raw& r, size_t) const { return load(r); }
    __device__ __forceinline__ uint32_t load(size_t pos) const {
        const ComposeArgs& a = b.a;
        const size_t B = (size_t)1 << a.log_b;
        const uint32_t f0 = f_at(pos), f1 = f_at(pos + B), f2 = f_at(pos + 2 * B);
        const uint32_t x = mont_mul(pow_lookup(a.htab, b.e0 + (uint32_t)pos), a.w_mont);
        return compose_eval<false>(a, f0, f1, f2, a.inv_xm1[pos], a.inv_xm1[pos + 2 * B], x, a.zz[pos & (B - 1)], a.first, a.last, a.alpha0_mont,
                                   a.alpha1g2_mont, 0u);
    }
};

struct ComposeBatchSrc {   // batch of proofs: leaf b*N + i = cp_b[i], with proof b's own challenges
    ComposeArgs a;
    const BatchChal* chal;
    using Raw = size_t;        // batched trees run with the chip full: nothing fetched ahead
    __device__ __forceinline__ Raw fetch(size_t pos) const { return pos; }
    __device__ __forceinline__ uint32_t finish(const Raw& r, size_t) const { return load(r); }
    __device__ __forceinline__ uint32_t load(size_t pos) const {
        const size_t b = pos >> a.logN, i = pos & (((size_t)1 << a.logN) - 1);
        const BatchChal c = chal[b];
        uint32_t v = compose_core<true>(a, a.f + (b << a.logN), c.first, c.last, c.alpha0_mont, c.alpha1g2_mont, c.alpha2_mont, i);
        a.cp[pos] = v;
        return v;
    }
};
struct FoldBatchSrc {      // leaf b*(m/2) + i = fold of proof b's layer with its own beta
    FoldArgs a;
    const BatchChal* chal;
    using Raw = size_t;
    __device__ __forceinline__ Raw fetch(size_t pos) const { return pos; }
    __device__ __forceinline__ uint32_t finish(const Raw& r, size_t) const { return load(r); }
    __device__ __forceinline__ uint32_t load(size_t pos) const {
        const uint32_t lh = a.log_m - 1;
        const size_t half = (size_t)1 << lh, b = pos >> lh, i = pos & (half - 1);
        const uint32_t* in = a.in + (b << a.log_m);
        uint32_t u = in[i], v = in[i + half];
        uint32_t xinv = pow_lookup(a.hinv, (uint32_t)(i << a.round));
        uint32_t s = mont_mul(add(u, v), a.inv2_mont);
        uint32_t d = mont_mul(mont_mul(sub(u, v), xinv), chal[b].c_mont);
        uint32_t r = add(s, d);
        a.out[pos] = r;
        return r;
    }
};

struct InterleaveSrc { // leaves arrive as 2^log_parts cyclic pieces of 2^log_cnt words (multi-GPU all-to-all output):
    const uint32_t* recv;  // leaf u*parts + q = recv[q*cnt + u]; hashed straight from the receive buffer
    uint32_t log_parts, log_cnt;
    using Raw = uint32_t;
    __device__ __forceinline__ uint32_t load(size_t pos) const {
        return recv[((pos & (((size_t)1 << log_parts) - 1)) << log_cnt) | (pos >> log_parts)];
    }
    __device__ __forceinline__ Raw fetch(size_t pos) const { return load(pos); }
    __device__ __forceinline__ uint32_t finish(const Raw& r, size_t) const { return r; }
};

// Sources whose constants may arrive after the launch was enqueued have a prepare(); every kernel calls it on its own copy of the
// source before the first element is produced.
template <class S> __device__ __forceinline__ auto src_prepare(S& s, int) -> decltype(s.prepare(), void()) { s.prepare(); }
template <class S> __device__ __forceinline__ void src_prepare(S&, long) {}

constexpr int kMerkleThreads = 256;
constexpr uint32_t kMerkleMaxK = 4;

__device__ __forceinline__ void store_digest(uint32_t* nodes, size_t node, const Digest& d) {
    uint4* q = reinterpret_cast<uint4*>(nodes + node * 8);
    q[0] = make_uint4(d.w[0], d.w[1], d.w[2], d.w[3]);
    q[1] = make_uint4(d.w[4], d.w[5], d.w[6], d.w[7]);
}
__device__ __forceinline__ Digest load_digest(const uint32_t* nodes, size_t node) {
    const uint4* q = reinterpret_cast<const uint4*>(nodes + node * 8);
    uint4 lo = q[0], hi = q[1];
    Digest d;
    d.w[0] = lo.x; d.w[1] = lo.y; d.w[2] = lo.z; d.w[3] = lo.w;
    d.w[4] = hi.x; d.w[5] = hi.y; d.w[6] = hi.z; d.w[7] = hi.w;
    return d;
}

__device__ __forceinline__ Digest lds_digest(const uint4* p) {
    uint4 lo = p[0], hi = p[1];
    Digest d;
    d.w[0] = lo.x; d.w[1] = lo.y; d.w[2] = lo.z; d.w[3] = lo.w;
    d.w[4] = hi.x; d.w[5] = hi.y; d.w[6] = hi.z; d.w[7] = hi.w;
    return d;
}

template <class SRC, bool LEAF, int HASH>
__global__ __launch_bounds__(kMerkleThreads) void merkle_subtree_kernel(SRC src, uint32_t* nodes,
                                                                        uint32_t depth_in, uint32_t k, size_t off) {
    // per wave: k pending LEFT sibling groups (one per level) + one scratch group for the right sibling of the
    // pairing in progress, 64 digests x 2 uint4 each = (k + 1) x 2 KiB: 40 KiB per workgroup at k = 4, four waves per
    // SIMD.  (Round 3 tried keeping only level 0 in LDS and re-reading the pending groups of higher levels from the
    // heap, where every digest is written anyway: 4 KiB per wave, <= 56 VGPRs, eight waves per SIMD and any k -- and
    // measured 6.19 ms per 2^24 proof against 6.07 ms for this kernel, profiles/r03_ab_subtree_heap.txt: SHA-256 as
    // compiled does not issue faster with more resident waves, and the second inlined copy of the hash costs more.)
    extern __shared__ __attribute__((aligned(16))) uint4 stage[];
    src_prepare(src, 0);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t gwave = (size_t)blockIdx.x * (kMerkleThreads / 64) + wave;
    // first input of this wave; `off` = position of a chunk's first node at this depth (0 for a whole
    // tree): a chunk is an aligned sub-range of the leaves, built into its place in the heap
    const size_t base = (gwave << (6 + k)) + off;
    const size_t in_base = ((size_t)1 << depth_in) - 1;
    uint4* my = stage + (size_t)wave * (k + 1) * 128;
    uint4* scratch = my + (size_t)k * 128;
    // The reads of group i + 1 are issued before group i is hashed (a wave that meets its load latency at the top of
    // every group stalls 2^k times, and with two waves per SIMD running the same code in step, both at once), and
    // they are consumed -- SRC::finish: the producer's arithmetic and the store of its value -- at the END of group i,
    // behind that group's digest stores: the wait in front of finish() then leaves those stores in flight.
    typename SRC::Raw raw;
    Digest dnext;
    uint32_t val = 0;
    if (LEAF) val = src.load(base + lane - off);                 // the source is chunk-local
    else dnext = load_digest(nodes, in_base + base + lane);
#pragma unroll 1
    for (uint32_t i = 0; i < (1u << k); ++i) {
        Digest d;
        const size_t pos = base + (size_t)i * 64 + lane;         // 64 consecutive inputs: coalesced
        const bool more = i + 1 < (1u << k);                     // wave-uniform
        if (LEAF) {
            if (more) raw = src.fetch(pos + 64 - off);
            d = Hasher<HASH>::leaf(val);
            store_digest(nodes, in_base + pos, d);
        } else {
            d = dnext;
            if (more) dnext = load_digest(nodes, in_base + pos + 64);
        }
        uint32_t idx = i, lvl = 0;
#pragma unroll 1
        while (lvl < k) {                                        // wave-uniform
            uint4* left = my + lvl * 128;
            uint4* grp = (idx & 1u) ? scratch : left;
            grp[2 * lane] = make_uint4(d.w[0], d.w[1], d.w[2], d.w[3]);
            grp[2 * lane + 1] = make_uint4(d.w[4], d.w[5], d.w[6], d.w[7]);
            if (!(idx & 1u)) break;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // children 2*lane, 2*lane+1 of the 128 buffered nodes: lanes 0-31 pair the left group, lanes 32-63 the right
            const uint4* x = (lane < 32u ? left : scratch - 128) + 4 * lane;
            Digest l = lds_digest(x), r = lds_digest(x + 2);
            __builtin_amdgcn_wave_barrier();
            d = Hasher<HASH>::inner(l, r);
            idx >>= 1;
            ++lvl;
            store_digest(nodes, (((size_t)1 << (depth_in - lvl)) - 1) + (base >> lvl) + (size_t)idx * 64 + lane, d);
        }
        if (LEAF && more) val = src.finish(raw, pos + 64 - off);
    }
}

// The throughput launch of a BLAKE2s tree.  The walk is merkle_subtree_kernel's, argument for argument: 64 * 2^k
// inputs per wave in groups of 64, sibling groups paired through the wave's (k + 1) x 2 KiB of LDS, every level on all 64 lanes, every
// digest stored once in a contiguous 2 KiB run -- so merkle_build_t plans one geometry for every hash.  It is a kernel of its own, not
// a third instantiation of that template, because the machine code of the SHA-256 and field-hash instances is pinned instruction for
// instruction (tests/test_kernel_descriptors.py) and must not move when this one is tuned.  One compression per node and no message
// schedule leave 16 + 16 live words in the hash; the next group's inputs (a leaf source's Raw, or the eight words of a digest) stay
// in flight across it exactly as there: fetch() ahead of the hash, finish() behind the group's digest stores.
// Only the sources the one-call prover reaches are instantiated (B2sSrc); the builds of the batched, sharded and chunked provers
// refuse the hash one level up.
template <class SRC> struct B2sSrc { static constexpr bool ok = false; };
template <> struct B2sSrc<PlainSrc> { static constexpr bool ok = true; };
template <> struct B2sSrc<ComposeSrc> { static constexpr bool ok = true; };
template <> struct B2sSrc<FoldSrc> { static constexpr bool ok = true; };

template <class SRC, bool LEAF>
__global__ __launch_bounds__(kMerkleThreads) void b2s_subtree_kernel(SRC src, uint32_t* nodes, uint32_t depth_in, uint32_t k, size_t off) {
    extern __shared__ __attribute__((aligned(16))) uint4 stage[];   // per wave: k pending left groups + the scratch group, 128 uint4 each
    src_prepare(src, 0);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t gwave = (size_t)blockIdx.x * (kMerkleThreads / 64) + wave;
    const size_t base = (gwave << (6 + k)) + off;                // first input of this wave (off: the chunk's first node at this depth)
    const size_t in_base = ((size_t)1 << depth_in) - 1;
    uint4* my = stage + (size_t)wave * (k + 1) * 128;
    uint4* scratch = my + (size_t)k * 128;
    typename SRC::Raw raw;
    Digest dnext;
    uint32_t val = 0;
    if (LEAF) val = src.load(base + lane - off);                 // the source is chunk-local
    else dnext = load_digest(nodes, in_base + base + lane);
#pragma unroll 1
    for (uint32_t i = 0; i < (1u << k); ++i) {
        Digest d;
        const size_t pos = base + (size_t)i * 64 + lane;         // 64 consecutive inputs: coalesced
        const bool more = i + 1 < (1u << k);                     // wave-uniform
        if (LEAF) {
            if (more) raw = src.fetch(pos + 64 - off);
            d = blake2s_leaf(val);
            store_digest(nodes, in_base + pos, d);
        } else {
            d = dnext;
            if (more) dnext = load_digest(nodes, in_base + pos + 64);
        }
        uint32_t idx = i, lvl = 0;
#pragma unroll 1
        while (lvl < k) {                                        // wave-uniform
            uint4* left = my + lvl * 128;
            uint4* grp = (idx & 1u) ? scratch : left;
            grp[2 * lane] = make_uint4(d.w[0], d.w[1], d.w[2], d.w[3]);
            grp[2 * lane + 1] = make_uint4(d.w[4], d.w[5], d.w[6], d.w[7]);
            if (!(idx & 1u)) break;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // children 2*lane, 2*lane+1 of the 128 buffered nodes: lanes 0-31 pair the left group, lanes 32-63 the right
            const uint4* x = (lane < 32u ? left : scratch - 128) + 4 * lane;
            const Digest l = lds_digest(x), r = lds_digest(x + 2);
            __builtin_amdgcn_wave_barrier();
            d = blake2s_inner(l, r);
            idx >>= 1;
            ++lvl;
            store_digest(nodes, (((size_t)1 << (depth_in - lvl)) - 1) + (base >> lvl) + (size_t)idx * 64 + lane, d);
        }
        if (LEAF && more) val = src.finish(raw, pos + 64 - off);
    }
}

// Latency-bound part of a tree.  A level with <= 65 536 nodes costs one hash latency however it
// is scheduled (one wave per SIMD already issues a VALU op every 4 cycles), so what matters here
// is the number of grid-wide synchronisations.  Each workgroup takes 2^j consecutive nodes of
// level `depth_in` (raw values in LEAF mode), keeps them in LDS and reduces them to ONE node with
// workgroup barriers only; a launch therefore lowers the tree by j levels.
constexpr int kWgThreads = 256;
#ifndef ZK_FIELD_ROW_MAX_NODES
#define ZK_FIELD_ROW_MAX_NODES 16       // round 6, re-swept with the quad form present (profiles/r06_ab_field_forms.txt): 32 nodes are one quad pass (5.3 us), not two row passes (7.2)
#endif
constexpr uint32_t kFieldRowMaxNodes = ZK_FIELD_ROW_MAX_NODES;   // levels of <= this many nodes per workgroup use the 16-lane row form of the field hash
static_assert(kFieldRowMaxNodes >= 16 && kFieldRowMaxNodes <= 64, "the row form takes at most four passes of 16 nodes");
#ifndef ZK_FIELD_QUAD_MAX_NODES
#define ZK_FIELD_QUAD_MAX_NODES 64      // profiles/r05_ab_field_quad.txt: 0 / 64 / 128 swept; a quad pass is ~6 us, so two of them lose to the one-lane hash
#endif
constexpr uint32_t kFieldQuadMaxNodes = ZK_FIELD_QUAD_MAX_NODES;   // ... of <= this many (and more than the row form's) one hash per quad of lanes; 0: never
static_assert(kFieldQuadMaxNodes <= 128, "the quad form takes at most two passes of 64 nodes");
#ifndef ZK_FIELD_ROW_LEAF_MAX
#define ZK_FIELD_ROW_LEAF_MAX 32        // 0: leaves always one lane per hash
#endif
constexpr uint32_t kFieldRowLeafMax = ZK_FIELD_ROW_LEAF_MAX;     // a workgroup with <= this many LEAVES of the field hash hashes them in the row form too (round 6)
static_assert(kFieldRowLeafMax <= 64, "the row form takes at most four passes of 16 leaves");
constexpr uint32_t kWgMaxLog = 10;   // 1024 digests = 32 KiB LDS per workgroup

__device__ __forceinline__ void lds_store(uint4* p, const Digest& d) {
    p[0] = make_uint4(d.w[0], d.w[1], d.w[2], d.w[3]);
    p[1] = make_uint4(d.w[4], d.w[5], d.w[6], d.w[7]);
}

// ---- handing a workgroup's result to the workgroup that finishes last (round 6) ----------------------------------------------
// The chip has eight compute dies with an L2 each.  Rounds 1-5 published a workgroup's node with an agent-scope RELEASE on the
// arrival counter (buffer_wbl2: write back the die's L2, ~0.5 MB of fresh digests per die in a 2^17-node launch) and the last
// workgroup took everything in with an ACQUIRE (buffer_inv).  tools/wg_trace.py put 5.4 - 8.3 us per latency launch between "a
// workgroup has its node" and "the last one starts the post" at EVERY tree size: that hand-over, not the hashing.  Only ONE node
// per workgroup has to cross: it is re-stored with eight write-through stores (relaxed atomic stores at agent scope: sc1), the
// wave waits for them, the counter is bumped RELAXED, and the last workgroup reads the nodes with agent-scope loads (sc1: they
// miss the die's L2).  Everything else a launch wrote becomes visible at the kernel boundary as always.
// Build-time A/B: ZK_BUILD_DEFS="-DZK_WG_RELAXED_PUBLISH=0" restores the release / acquire form.
#ifndef ZK_WG_RELAXED_PUBLISH
#define ZK_WG_RELAXED_PUBLISH 1
#endif
constexpr bool kWgRelaxedPublish = ZK_WG_RELAXED_PUBLISH != 0;
__device__ __forceinline__ void publish_node(uint32_t* nodes, size_t node, const uint4* lvl0, uint32_t tid) {
    if (tid < 8) __hip_atomic_store(nodes + node * 8 + tid, reinterpret_cast<const uint32_t*>(lvl0)[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // wave 0: the eight stores are out before its thread 0 counts
}
__device__ __forceinline__ Digest load_digest_agent(const uint32_t* nodes, size_t node) {
    // four 8-byte agent-scope loads (global_load_dwordx2 ... sc1; a digest is 32-byte aligned)
    const unsigned long long* q = reinterpret_cast<const unsigned long long*>(nodes + node * 8);
    Digest d;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned long long v = __hip_atomic_load(q + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        d.w[2 * i] = (uint32_t)v; d.w[2 * i + 1] = (uint32_t)(v >> 32);
    }
    return d;
}

// ---- diagnostic build: where the time of a latency launch goes (ZK_BUILD_DEFS="-DZK_WG_TRACE=1"; tools/wg_trace.py) ----------
// Thread 0 of workgroup 0 stamps the 100 MHz constant clock (s_memrealtime: one time base for every compute unit) at entry,
// after the inputs are in LDS, and after every level; the workgroup that carries on (continuation) and the one that posts to the
// host stamp their steps into the same record.  Records are dumped to $ZK_WG_TRACE_FILE when a context is destroyed.  Not part
// of a product build: the stamps cost a scalar memory-time read and a store per level.
#ifdef ZK_WG_TRACE
constexpr uint32_t kWgTraceSlots = 48, kWgTraceLaunches = 8192;
__device__ unsigned long long g_wg_trace[kWgTraceLaunches][kWgTraceSlots];
__device__ unsigned int g_wg_trace_n, g_wg_trace_cur;
#define WG_STAMP(slot) do { if (threadIdx.x == 0 && wg_rec < kWgTraceLaunches && (slot) < kWgTraceSlots) g_wg_trace[wg_rec][(slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define WG_STAMP(slot) do { } while (0)
#endif

// When the launch reaches the hand-over depth (MailArgs.top; 0 = the root) and a mailbox is given, the
// digests of that depth are also written to host-mapped memory followed by a sequence number, so the
// host prover can poll for them instead of paying a blit kernel + stream synchronisation per commitment.
// j2 > 0 (whole trees only, mail.counter given): the workgroup that finishes LAST goes on with the gridDim.x nodes the
// launch has produced (<= 2^kWgMaxLog of them) and lowers the tree by j2 more levels -- one launch where the levels of a
// tree used to need two (round 5: the field hash, which hands nothing to the host, paid 38 latency launches per proof).
template <class SRC, bool LEAF, int HASH>
__global__ __launch_bounds__(kWgThreads) void merkle_wg_kernel(SRC src, uint32_t* nodes, uint32_t depth_in, uint32_t j,
                                                               MailArgs mail, size_t off, uint32_t j2, uint32_t lds_log) {
    extern __shared__ __attribute__((aligned(16))) uint4 lvl[];   // [2^lds_log][2], then the 16 KiB schedule exchange
    src_prepare(src, 0);
    uint32_t* xch = reinterpret_cast<uint32_t*>(lvl + ((size_t)2 << lds_log));
    const uint32_t tid = threadIdx.x;
    uint32_t cnt = 1u << j;                                       // inputs of this workgroup in the current phase
    size_t first = ((size_t)blockIdx.x << j) + off;               // first input of this workgroup (off: see merkle_subtree_kernel)
    uint32_t d_in = depth_in, lv = j;                             // the current phase lowers depth d_in by lv levels
    const size_t in_base = ((size_t)1 << depth_in) - 1;
    QuadLane ql;
    if (HASH == 0) ql = quad_lane(tid);
#ifdef ZK_WG_TRACE
    uint32_t wg_rec = 0xffffffffu;                                // record of this launch; only workgroup 0 knows it until the hand-over
    if (blockIdx.x == 0 && tid == 0) {
        wg_rec = atomicAdd(&g_wg_trace_n, 1u);
        __hip_atomic_store(&g_wg_trace_cur, wg_rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (wg_rec < kWgTraceLaunches) {
            for (uint32_t i = 0; i < kWgTraceSlots; ++i) g_wg_trace[wg_rec][i] = 0;
            g_wg_trace[wg_rec][0] = (unsigned long long)depth_in | ((unsigned long long)j << 8) | ((unsigned long long)j2 << 16) | ((unsigned long long)(LEAF ? 1 : 0) << 24) |
                                    ((unsigned long long)HASH << 25) | ((unsigned long long)(mail.mailbox ? mail.top + 1 : 0) << 26) | ((unsigned long long)gridDim.x << 32);
        }
    }
    WG_STAMP(1);
#endif
    // a thread takes up to 2^kWgMaxLog / kWgThreads = 4 inputs: every read is issued before the first one is used (one
    // load latency per launch instead of one per input; this phase is a chain of latencies)
    constexpr uint32_t kPer = (1u << kWgMaxLog) / kWgThreads;
    if (LEAF && HASH == 1 && cnt <= kFieldRowLeafMax) {
        // Few leaves of the field hash (the small trees of a proof's tail, spread over several workgroups): a leaf is the same
        // permutation as a node, on (v, 0, ..., 0, 1), so it takes the 16-lane row form as well -- 3.6 us per pass of 16 leaves where
        // the one-lane hash costs ~10.7 us however few there are (profiles/r06_wg_trace_21_field.txt: "load/leaf" of every leaf-mode
        // launch).  Every lane of a row asks the source for the row's leaf (one address: the loads coalesce; a fused producer computes
        // and stores the same value sixteen times over, which costs lanes that would idle anyway).
        const uint32_t g = tid & 15u, grp = tid >> 4;
#pragma unroll 1
        for (uint32_t b = 0; b * 16 < cnt; ++b) {
            const uint32_t i = b * 16 + grp;
            const uint32_t ii = i < cnt ? i : 0u;                  // idle rows recompute leaf 0 (DPP needs whole rows running)
            const uint32_t v = src.finish(src.fetch(first + ii - off), first + ii - off);
            const uint32_t word = g == 0 ? v : g == 15 ? 1u : 0u;
            const uint32_t res = fieldhash_inner_row16_f64(word, g, g_fh_consts64);
            if (i < cnt && g < 8) {
                nodes[(in_base + first + i) * 8 + g] = res;
                reinterpret_cast<uint32_t*>(&lvl[2 * i])[g] = res;
            }
        }
    } else if (LEAF) {
        typename SRC::Raw raw[kPer] = {};
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u)
            if (tid + u * kWgThreads < cnt) raw[u] = src.fetch(first + tid + u * kWgThreads - off);
#pragma unroll 1
        for (uint32_t i = tid; i < cnt; i += kWgThreads) {          // one copy of the hash: the fetched inputs move up
            const Digest d = Hasher<HASH>::leaf(src.finish(raw[0], first + i - off));
            store_digest(nodes, in_base + first + i, d);
            lds_store(&lvl[2 * i], d);
#pragma unroll
            for (uint32_t u = 0; u + 1 < kPer; ++u) raw[u] = raw[u + 1];
        }
    } else {
        Digest dd[kPer];
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u)
            if (tid + u * kWgThreads < cnt) dd[u] = load_digest(nodes, in_base + first + tid + u * kWgThreads);
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u)
            if (tid + u * kWgThreads < cnt) lds_store(&lvl[2 * (tid + u * kWgThreads)], dd[u]);
    }
    // the layer values this workgroup produced are read by ANOTHER workgroup (the one that finishes last) when
    // they are posted to the host: make every wave's stores visible device-wide, not only the posting wave's
    if (LEAF && mail.dump_src) __threadfence();
    __syncthreads();
    WG_STAMP(2);
#pragma unroll 1
  for (uint32_t phase = 0;; ++phase) {
#pragma unroll 1
    for (uint32_t t = 1; t <= lv; ++t) {
        const uint32_t w = cnt >> t;                              // nodes of this level in the workgroup
        const size_t out_base = (((size_t)1 << (d_in - t)) - 1) + (first >> t);
        WG_STAMP((phase ? 24u : 2u) + t - 1u);                   // start of level t = end of level t - 1
        if (HASH == 0 && w <= 64) {
            // Latency-bound level of <= 64 nodes per workgroup: one SHA-256 per FOUR lanes (sha256_quad.hpp: ~1 700
            // instructions on the wave instead of 2 293, no exchange inside the hash), 16 hashes per wave, the waves of
            // the workgroup side by side on their own SIMDs.  Every lane of a wave that hashes runs the code (DPP).
            const uint32_t lane = tid & 63u, wave = tid >> 6;
            const uint32_t node = wave * 16 + (lane >> 4) * 4 + (lane & 3u), role = (lane >> 2) & 3u;
            const bool busy = wave * 16 < w;                          // wave-uniform
            uint32_t o[4];
            if (busy) sha256_inner_quad(reinterpret_cast<const uint32_t*>(&lvl[4 * (node < w ? node : 0u)]), ql, o);
            __syncthreads();                                       // every read of the level done
            if (busy && node < w && role < 2) {                    // bank 1 holds words 0-3, bank 0 words 4-7
                const uint4 v = make_uint4(o[0], o[1], o[2], o[3]);
                lvl[2 * node + (role ^ 1u)] = v;
                reinterpret_cast<uint4*>(nodes + (out_base + node) * 8)[role ^ 1u] = v;
            }
            __syncthreads();
            continue;
        }
        if (HASH == 0 && w <= 128) {
            // Latency-bound level with idle waves: split each SHA-256 between a main lane (waves 0-1:
            // the 2 x 64 rounds) and a helper lane (waves 2-3: the 48 message-schedule steps of block 1),
            // 16 rounds at a time through a double-buffered LDS exchange.  The main lane's critical
            // path drops from 2293 to ~1850 instructions.
            const bool is_main = tid < 128;
            const uint32_t node = tid & 127u;
            const bool active = node < w;
            uint32_t wv[16];
            uint32_t st[8];
            if (active) {
                Digest l = lds_digest(&lvl[4 * node]), r = lds_digest(&lvl[4 * node + 2]);
#pragma unroll
                for (int i = 0; i < 8; ++i) { wv[i] = l.w[i]; wv[8 + i] = r.w[i]; st[i] = SHA_IV[i]; }
            }
            uint32_t* xb0 = xch;                                   // [16][128]
            uint32_t* xb1 = xch + 16 * 128;
            // phase A: rounds 0-15 | W16-31 -> xb0
            if (active) {
                if (is_main) sha256_rounds16<0>(st, wv);
                else { sha256_schedule16(wv);
#pragma unroll
                       for (int i = 0; i < 16; ++i) xb0[i * 128 + node] = wv[i]; }
            }
            __syncthreads();
            // phase B: rounds 16-31 | W32-47 -> xb1
            if (active) {
                if (is_main) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) wv[i] = xb0[i * 128 + node];
                    sha256_rounds16<16>(st, wv);
                } else { sha256_schedule16(wv);
#pragma unroll
                         for (int i = 0; i < 16; ++i) xb1[i * 128 + node] = wv[i]; }
            }
            __syncthreads();
            // phase C: rounds 32-47 | W48-63 -> xb0
            if (active) {
                if (is_main) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) wv[i] = xb1[i * 128 + node];
                    sha256_rounds16<32>(st, wv);
                } else { sha256_schedule16(wv);
#pragma unroll
                         for (int i = 0; i < 16; ++i) xb0[i * 128 + node] = wv[i]; }
            }
            __syncthreads();
            // phase D: rounds 48-63, feed-forward, padding block
            Digest d0;
            if (active && is_main) {
#pragma unroll
                for (int i = 0; i < 16; ++i) wv[i] = xb0[i * 128 + node];
                sha256_rounds16<48>(st, wv);
#pragma unroll
                for (int i = 0; i < 8; ++i) d0.w[i] = st[i] + SHA_IV[i];
                uint32_t pad[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 512u};
                sha256_compress(d0.w, pad);
            }
            __syncthreads();                                       // every read of lvl and xch done
            if (active && is_main) { lds_store(&lvl[2 * node], d0); store_digest(nodes, out_base + node, d0); }
            __syncthreads();
            continue;
        }
        if (HASH == 1 && w > kFieldRowMaxNodes && w <= kFieldQuadMaxNodes) {
            // Level of 33 .. 64 nodes per workgroup of the field hash: one hash per QUAD of lanes (fieldhash_inner_quad_f64: a
            // 4-block of the state per lane, ~1 950 instructions, ~6 us), 64 hashes per pass of the workgroup.  Lane q reads children
            // words 4q .. 4q+3 as one 16-byte LDS access; lanes 0 and 1 of a quad hold the digest.
            const uint32_t q = tid & 3u, grp = tid >> 2;
            uint32_t res[2][4];
#pragma unroll
            for (uint32_t b = 0; b < 2; ++b) {
                if (b * 64 >= w) break;                                // workgroup-uniform
                const uint32_t node = b * 64 + grp;
                const uint4 v = lvl[4 * (node < w ? node : 0u) + q];
                const uint32_t in[4] = {v.x, v.y, v.z, v.w};
                fieldhash_inner_quad_f64(in, q, res[b], g_fh_consts64);
            }
            __syncthreads();                                       // every read of the level done
#pragma unroll
            for (uint32_t b = 0; b < 2; ++b) {
                if (b * 64 >= w) break;
                const uint32_t node = b * 64 + grp;
                if (node < w && q < 2) {
                    const uint4 o = make_uint4(res[b][0], res[b][1], res[b][2], res[b][3]);
                    lvl[2 * node + q] = o;
                    reinterpret_cast<uint4*>(nodes + (out_base + node) * 8)[q] = o;
                }
            }
            __syncthreads();
            continue;
        }
        if (HASH == 1 && w <= kFieldRowMaxNodes) {
            // Narrow level of the field hash: one hash per ROW of 16 lanes in double precision (fieldhash_inner_row16_f64: the 16
            // state elements on 16 lanes, quad broadcasts and row rotations, ~1 170 instructions), 16 hashes per pass of the
            // workgroup, 3.9 us per pass (the 32-bit row form of rounds 3-4: 5.4); the one-lane hash takes ~11 us for up to 256
            // nodes, so the row form pays up to 32 nodes per workgroup (profiles/r05_ab_field_row.txt: 16 / 32 / 64 swept).
            // Every lane runs the permutation (DPP needs whole rows).
            const uint32_t g = tid & 15u, grp = tid >> 4;
            uint32_t res[4];
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                if (b * 16 >= w) break;                                // workgroup-uniform
                const uint32_t node = b * 16 + grp;
                const uint32_t* words = reinterpret_cast<const uint32_t*>(&lvl[4 * (node < w ? node : 0u)]);   // children 2 node, 2 node + 1
                res[b] = fieldhash_inner_row16_f64(words[g], g, g_fh_consts64);
            }
            __syncthreads();                                       // every read of the level done
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                if (b * 16 >= w) break;
                const uint32_t node = b * 16 + grp;
                if (node < w && g < 8) {
                    reinterpret_cast<uint32_t*>(&lvl[2 * node])[g] = res[b];
                    nodes[(out_base + node) * 8 + g] = res[b];
                }
            }
            __syncthreads();
            continue;
        }
        // in place: node u is written over child slot u after every thread of the level has read
        Digest d0, d1;
        const bool a0 = tid < w, a1 = tid + kWgThreads < w;       // w <= 512: at most two nodes per thread
        if (a0) d0 = Hasher<HASH>::inner(lds_digest(&lvl[4 * tid]), lds_digest(&lvl[4 * tid + 2]));
        if (a1) d1 = Hasher<HASH>::inner(lds_digest(&lvl[4 * (tid + kWgThreads)]), lds_digest(&lvl[4 * (tid + kWgThreads) + 2]));
        __syncthreads();
        if (a0) { lds_store(&lvl[2 * tid], d0); store_digest(nodes, out_base + tid, d0); }
        if (a1) { lds_store(&lvl[2 * (tid + kWgThreads)], d1); store_digest(nodes, out_base + tid + kWgThreads, d1); }
        __syncthreads();
    }
    WG_STAMP((phase ? 24u : 2u) + lv);                           // end of the last level of this phase
    if (phase == 1 || j2 == 0) break;
    // Continuation.  Every workgroup has written its node of depth depth_in - j (the barrier that ends a level has drained
    // the stores of all its waves); an agent-scope release / acquire on a counter tells the one that arrives last, and that
    // one alone reads the gridDim.x nodes back (the acquire has invalidated its CU's vector L1) and carries on.
    __shared__ uint32_t go_on;
    if (gridDim.x > 1) {
        if (kWgRelaxedPublish) {
            // this workgroup's node (lvl[0..1] after the last level) goes out write-through; nothing else has to cross dies
            publish_node(nodes, (((size_t)1 << (depth_in - j)) - 1) + blockIdx.x, lvl, tid);
        } else {
            // every wave's digest stores have reached L2 before thread 0 releases them to the other compute dies: a wait on this
            // wave's own stores, then the barrier; the agent-scope release itself (an L2 write-back) is paid ONCE per workgroup,
            // by the atomic below (256 workgroups x 4 waves of agent-scope fences cost the SHA-256 path 4 us per tree)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    if (tid == 0) {
        uint32_t last = 1;
        if (gridDim.x > 1) {
            last = (kWgRelaxedPublish ? __hip_atomic_fetch_add(mail.counter + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                      : __hip_atomic_fetch_add(mail.counter + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT)) == gridDim.x - 1;
            if (last) __hip_atomic_store(mail.counter + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        go_on = last;
    }
    __syncthreads();
    if (!go_on) return;                                            // workgroup-uniform
    // a launch that also posts layer values (once per proof): the values the OTHER workgroups stored (behind their __threadfence
    // above) are read by this one with ordinary loads at the end -- take them in with an acquire, as the counter did in rounds 1-5
    if (kWgRelaxedPublish && LEAF && mail.dump_src) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#ifdef ZK_WG_TRACE
    if (tid == 0) wg_rec = __hip_atomic_load(&g_wg_trace_cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // workgroup 0 wrote it before it reached the counter
    WG_STAMP(15);
#endif
    d_in = depth_in - j; lv = j2; cnt = gridDim.x; first = 0;
    {
        const size_t base2 = ((size_t)1 << d_in) - 1;
        Digest dd[kPer];
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u)
            if (tid + u * kWgThreads < cnt)
                dd[u] = (kWgRelaxedPublish && gridDim.x > 1) ? load_digest_agent(nodes, base2 + tid + u * kWgThreads) : load_digest(nodes, base2 + tid + u * kWgThreads);
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u)
            if (tid + u * kWgThreads < cnt) lds_store(&lvl[2 * (tid + u * kWgThreads)], dd[u]);
    }
    __syncthreads();
    WG_STAMP(16);
  }
    // The launch that reaches depth mail.top posts its 2^top digests (and, on request, the layer values) to the
    // host: small PCIe writes are slow, so the workgroup that finishes last copies everything with wide stores.
    if (mail.mailbox && depth_in - j - j2 == mail.top && off == 0) {
        __shared__ uint32_t is_last;
        // one node per workgroup crosses the dies write-through (publish_node); a launch that also posts layer values keeps the
        // release / acquire form, which covers them as well (once per proof: the layer that feeds the host's FRI tail)
        const bool relaxed = kWgRelaxedPublish && gridDim.x > 1 && j2 == 0 && mail.dump_src == nullptr;   // uniform over the launch
        if (relaxed) publish_node(nodes, (((size_t)1 << mail.top) - 1) + blockIdx.x, lvl, tid);
        if (tid == 0) {
            uint32_t last = 1;
            if (gridDim.x > 1 && j2 == 0) {                        // with a continuation only the last workgroup gets here
                // release: this workgroup's digest (and values) are out; acquire: so are everybody else's
                last = (relaxed ? __hip_atomic_fetch_add(mail.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                : __hip_atomic_fetch_add(mail.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT)) == gridDim.x - 1;
                if (last) __hip_atomic_store(mail.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            is_last = last;
        }
        __syncthreads();
        if (is_last) {
#ifdef ZK_WG_TRACE
            if (tid == 0 && wg_rec == 0xffffffffu) wg_rec = __hip_atomic_load(&g_wg_trace_cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            WG_STAMP(40);
#endif
            const uint4* sq = reinterpret_cast<const uint4*>(nodes + (((size_t)1 << mail.top) - 1) * 8);
            uint4* dq = reinterpret_cast<uint4*>(mail.mailbox + kMailDigests);
            if (relaxed) {                                         // the peers' nodes: agent-scope loads (they are not in this die's L2)
                for (uint32_t i = tid; i < (1u << mail.top); i += kWgThreads) {
                    const Digest d = load_digest_agent(nodes, (((size_t)1 << mail.top) - 1) + i);
                    dq[2 * i] = make_uint4(d.w[0], d.w[1], d.w[2], d.w[3]);
                    dq[2 * i + 1] = make_uint4(d.w[4], d.w[5], d.w[6], d.w[7]);
                }
            } else {
                for (uint32_t i = tid; i < (2u << mail.top); i += kWgThreads) dq[i] = sq[i];
            }
            if (mail.dump_src) {
                const uint4* sv = reinterpret_cast<const uint4*>(mail.dump_src);
                uint4* dv = reinterpret_cast<uint4*>(mail.mailbox + mail.vals_off);
                for (uint32_t i = tid; i < (1u << mail.dump_log) / 4; i += kWgThreads) dv[i] = sv[i];
            }
            __threadfence_system();
            __syncthreads();
            WG_STAMP(41);
            if (tid == 0) __hip_atomic_store(&mail.mailbox[0], mail.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            WG_STAMP(42);
        }
    }
}

#ifdef ZK_WG_TRACE
// Appends the records collected so far to $ZK_WG_TRACE_FILE (one line per latency launch) and clears them; called when a context
// is destroyed.  meta: depth_in, j, j2, leaf, hash, hand-over depth + 1 (0: no mailbox), workgroups; then the stamps in 10 ns ticks
// relative to the launch's first stamp (0 = not reached).
void dump_wg_trace() {
    const char* path = getenv("ZK_WG_TRACE_FILE");
    unsigned int n = 0;
    if (!path || hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_wg_trace_n), sizeof n) != hipSuccess || !n) return;
    if (n > kWgTraceLaunches) n = kWgTraceLaunches;
    std::vector<unsigned long long> rec((size_t)n * kWgTraceSlots);
    if (hipMemcpyFromSymbol(rec.data(), HIP_SYMBOL(g_wg_trace), rec.size() * 8) != hipSuccess) return;
    FILE* f = fopen(path, "a");
    if (!f) return;
    for (unsigned int r = 0; r < n; ++r) {
        const unsigned long long* x = &rec[(size_t)r * kWgTraceSlots];
        const unsigned long long m = x[0];
        fprintf(f, "wg depth_in=%llu j=%llu j2=%llu leaf=%llu hash=%llu top=%lld wgs=%llu abs0=%llu :", m & 255, (m >> 8) & 255, (m >> 16) & 255, (m >> 24) & 1, (m >> 25) & 1,
                (long long)((m >> 26) & 63) - 1, m >> 32, x[1]);
        for (uint32_t i = 1; i < kWgTraceSlots; ++i) fprintf(f, " %lld", x[i] ? (long long)(x[i] - x[1]) : -1LL);
        fprintf(f, "\n");
    }
    fclose(f);
    const unsigned int zero = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wg_trace_n), &zero, sizeof zero);
}
#endif

// ---- coset leaves (transcript.hpp "coset") -------------------------------------------------------------------
// Leaf c of the tree over a layer of 2^log_len values holds the s = 2^STEPS values layer[c + u len / s], u < s: what one query
// opens in that layer.  A lane owns leaves c, c + stride, ...: its s loads are s coalesced runs across the wave (the layer stays
// in natural order), the values of its NEXT leaf are in flight while it hashes the current one (the fetch / finish split of the
// leaf sources), and a leaf is ONE compression whatever s: SHA-256 of 4 s <= 32 bytes is a single block whose padding words fold
// away in the schedule, BLAKE2s-256 of the same message is one compression whose zero words fold away, the field hash takes the
// state (slot_0 .. slot_{s-1}, 0, ..., 0, s).  s = 1 is Hasher::leaf.  The digest
// goes to heap position len / s - 1 + c; the levels above are built from there by the inner kernels (launch_merkle_build_coset).
template <int HASH, int S>
__device__ __forceinline__ Digest coset_leaf_digest(const uint32_t (&v)[S]) {
    Digest d;
    if (HASH == ZK_HASH_BLAKE2S) {
        d = blake2s_slots<S>(v);
    } else if (HASH == ZK_HASH_FIELD) {
        uint32_t in[kFhT];
#pragma unroll
        for (int i = 0; i < kFhT; ++i) in[i] = i < S ? v[i] : 0u;
        in[kFhT - 1] = (uint32_t)S;
        fh64_compress(in, d.w, g_fh_consts64);
    } else {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = i < S ? v[i] : 0u;
        w[S] = 0x80000000u;
        w[15] = 32u * S;
#pragma unroll
        for (int i = 0; i < 8; ++i) d.w[i] = SHA_IV[i];
        sha256_compress(d.w, w);
    }
    return d;
}
constexpr int kCosetThreads = 256;
template <int HASH, int STEPS>
__global__ __launch_bounds__(kCosetThreads) void coset_leaf_hash_kernel(const uint32_t* __restrict__ layer, uint32_t log_len, uint32_t* __restrict__ nodes) {
    constexpr int S = 1 << STEPS;
    const size_t leaves = (size_t)1 << (log_len - STEPS);        // also the distance between two slots of a leaf
    const size_t stride = (size_t)gridDim.x * kCosetThreads;     // a power of two <= leaves, or one workgroup: every lane of a wave makes the same trips
    size_t c = (size_t)blockIdx.x * kCosetThreads + threadIdx.x;
    if (c >= leaves) return;
    uint32_t v[S], nx[S] = {};
#pragma unroll
    for (int u = 0; u < S; ++u) v[u] = layer[c + (size_t)u * leaves];
    bool more;
#pragma unroll 1
    do {
        const size_t cn = c + stride;
        more = cn < leaves;
        if (more) {
#pragma unroll
            for (int u = 0; u < S; ++u) nx[u] = layer[cn + (size_t)u * leaves];
        }
        store_digest(nodes, leaves - 1 + c, coset_leaf_digest<HASH, S>(v));
#pragma unroll
        for (int u = 0; u < S; ++u) v[u] = nx[u];
        c = cn;
    } while (more);
}

static double merkle_bytes(bool leaf, uint32_t depth, uint32_t k) {
    // inputs read once (4 B values or 32 B digests), every produced digest written once
    double in = (double)((size_t)1 << depth);
    double produced = (leaf ? in : 0.0) + in * (1.0 - 1.0 / (double)((size_t)1 << k));
    return (leaf ? 4.0 : 32.0) * in + 32.0 * produced;
}
static double hash_leaf_ops(int hash) { return hash == ZK_HASH_FIELD ? kFieldLeafOps : hash == ZK_HASH_BLAKE2S ? kB2sLeafOps : kShaLeafOps; }
static double merkle_ops(bool leaf, uint32_t depth, uint32_t k, int hash) {
    double in = (double)((size_t)1 << depth);
    double lo = hash_leaf_ops(hash), io = hash == ZK_HASH_FIELD ? kFieldInnerOps : hash == ZK_HASH_BLAKE2S ? kB2sInnerOps : kShaInnerOps;
    return (leaf ? in * lo : 0.0) + in * (1.0 - 1.0 / (double)((size_t)1 << k)) * io;
}

static hipError_t ensure_fieldhash_consts() {
    static bool done[64] = {false};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || done[dev]) return hipSuccess;
    FieldHashConsts c;
    fieldhash_make_consts(c);
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_fh_consts), &c, sizeof c);
    if (e != hipSuccess) return e;
    static FieldHashConsts64 c64;
    fieldhash_make_consts64(c, c64);
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_fh_consts64), &c64, sizeof c64);
    if (e == hipSuccess) done[dev] = true;
    return e;
}

// Throughput phase: subtree launches (k <= 4 levels each) while the level has more than 2^18 nodes,
// i.e. while there are more than ~4 waves per SIMD to keep busy.  Latency phase: workgroup launches
// of up to 10 levels each.
// Build-time constants (ZK_BUILD_DEFS="-DZK_MERKLE_MAX_K=3" to A/B them; profiles/r03_ab_max_k.txt, r03_config2_switches.txt):
// levels per subtree launch, and the level size at which the throughput phase hands over to the latency phase (measured
// flat optimum 2^16 .. 2^18 nodes).  The hand-over depth can also be moved at run time with zk_dev_set_merkle_latency_log
// (include/zkstark_amd.h: tests use it to drive small trees through the chunked build).
#ifndef ZK_MERKLE_MAX_K
#define ZK_MERKLE_MAX_K 4
#endif
#ifndef ZK_MERKLE_LATENCY_LOG
#define ZK_MERKLE_LATENCY_LOG 17
#endif
#ifndef ZK_MERKLE_CHUNK_K
#define ZK_MERKLE_CHUNK_K 3
#endif
static_assert(ZK_MERKLE_MAX_K >= 1 && ZK_MERKLE_MAX_K <= (int)kMerkleMaxK && ZK_MERKLE_CHUNK_K >= 1 && ZK_MERKLE_CHUNK_K <= (int)kMerkleMaxK, "levels per launch");
static_assert(ZK_MERKLE_LATENCY_LOG >= 12 && ZK_MERKLE_LATENCY_LOG <= 24, "latency switch");
static uint32_t g_merkle_latency_log = ZK_MERKLE_LATENCY_LOG;
static constexpr uint32_t merkle_max_k() { return ZK_MERKLE_MAX_K; }
static uint32_t merkle_latency_log() { return __atomic_load_n(&g_merkle_latency_log, __ATOMIC_RELAXED); }
bool set_merkle_latency_log(uint32_t v) {
    if (v == 0) v = ZK_MERKLE_LATENCY_LOG;
    if (v < 12 || v > 24) return false;
    __atomic_store_n(&g_merkle_latency_log, v, __ATOMIC_RELAXED);
    return true;
}

// ---- how the latency phase of a tree is cut into (phase 1, continuation) -------------------------------------------
// Microseconds one workgroup, alone on its compute unit, needs for a level of w nodes (every form costs one hash LATENCY per
// pass: measured per form): SHA-256 one lane per hash 4.6 (256 per pass), main / helper lanes 4.9 (128),
// four lanes per hash 3.1 (64); field hash one lane per hash in double precision ~11 (256 per pass; tools/fh64_probe.hip: 10.7 us
// on a lone wave), a row of 16 lanes in double precision 3.9 (16 per pass; the 32-bit row form of rounds 3-4: 5.4).
// BLAKE2s one lane per hash: DERIVED, not traced -- its instruction count times the time per instruction of the SHA-256 one-lane entry
// (4.6 us / kShaInnerOps for a node, 2.6 us / kShaLeafOps for a leaf), 256 per pass; to be replaced by a trace (tools/wg_trace.py).
constexpr double kB2sLevelUs = kB2sInnerOps * 4.6 / kShaInnerOps, kB2sLeafUs = kB2sLeafOps * 2.6 / kShaLeafOps;
static double wg_level_us(uint32_t w, int hash) {
    if (w == 0) return 0.0;
    if (hash == ZK_HASH_BLAKE2S) return (double)((w + 255) / 256) * kB2sLevelUs;
    if (hash == ZK_HASH_FIELD) return w <= kFieldRowMaxNodes ? (double)((w + 15) / 16) * 3.7 : w <= kFieldQuadMaxNodes ? (double)((w + 63) / 64) * 5.3 : (double)((w + 255) / 256) * 10.8;   // round 6: as traced (tools/wg_trace.py)
    return w <= 64 ? 3.1 : w <= 128 ? 4.9 : (double)((w + 255) / 256) * 4.6;
}
static double wg_phase_us(bool leaf, uint32_t cnt_log, uint32_t levels, int hash, uint32_t blocks) {
    const uint32_t cnt = 1u << cnt_log;
    double us = !leaf ? 1.0                                                        // the first load, or the leaf hashes:
                : hash == ZK_HASH_FIELD ? (cnt <= kFieldRowLeafMax ? (double)((cnt + 15) / 16) * 3.7 : (double)((cnt + 255) / 256) * 10.8)
                : (double)((cnt + 255) / 256) * (hash == ZK_HASH_BLAKE2S ? kB2sLeafUs : 2.6);
    for (uint32_t t = 1; t <= levels; ++t) us += wg_level_us(cnt >> t, hash);
    return blocks > 256 ? us * (double)blocks / 256.0 : us;                        // more workgroups than compute units take turns
}
// Build-time A/B switch (ZK_BUILD_DEFS="-DZK_MERKLE_CONTINUATION=0": one launch per <= 10 levels, as rounds 1-4)
#ifndef ZK_MERKLE_CONTINUATION
#define ZK_MERKLE_CONTINUATION 1
#endif
static constexpr bool g_merkle_continuation = ZK_MERKLE_CONTINUATION != 0;
constexpr double kContinueUs = 6.0;    // the continuation's release -> count -> acquire -> reload
constexpr double kLaunchUs = 10.0;     // a further launch on the commit -> challenge -> launch path

// Builds the levels of a heap over 2^log_m leaves that lie above the aligned leaf range
// [chunk << log_sub, (chunk + 1) << log_sub), from the leaves (leaf_mode) or from the nodes already
// present at depth `log_m - log_sub + span` ... up to the chunk's own root at depth log_m - log_sub.
// A whole tree is chunk 0 with log_sub = log_m.
template <class SRC>
static hipError_t merkle_build_t(SRC src, double src_bytes, uint32_t log_m, uint32_t* nodes, hipStream_t s, Profiler* prof,
                                 const MailArgs& mail_in, int hash, uint32_t log_sub = 0xffffffffu, size_t chunk = 0,
                                 bool leaf_mode = true, uint32_t tp_floor = 0) {
    if (hash == ZK_HASH_BLAKE2S && !B2sSrc<SRC>::ok) return hipErrorInvalidValue;   // only the one-call prover's sources (b2s_subtree_kernel)
    if (hash == ZK_HASH_FIELD) {
        hipError_t e = ensure_fieldhash_consts();
        if (e != hipSuccess) return e;
    }
    if (log_sub == 0xffffffffu) log_sub = log_m;
    const uint32_t stop = log_m - log_sub;            // depth of the chunk root
    uint32_t depth = log_m;
    bool leaf = leaf_mode;
    const PlainSrc none{nullptr};
    // the first launch reads its leaves through SRC: replace the plain 4 B/leaf read by the source's bytes
    auto first_bytes = [&](double b) { return leaf ? b - 4.0 * (double)((size_t)1 << log_sub) + src_bytes : b; };
    const uint32_t kMerkleLatencyLog = merkle_latency_log();
    auto off_at = [&](uint32_t d) { return (size_t)chunk << (d - stop); };   // chunk's first node at depth d
    // a chunk build (tp_floor != 0) runs the subtree kernels down to that ABSOLUTE depth and stops there;
    // launch_merkle_finish builds everything above it once, for the whole tree
    const bool throughput_only = tp_floor != 0;
    // top > 0 (whole trees only): the build ends at depth `top`, whose 2^top digests go to the mailbox and the
    // levels above are hashed by the host (host_sha.hpp; batches: those digests are the per-proof roots).  Without a mailbox the
    // build just ends there (a batch's caps deeper than the mailbox holds: launch_digest_level_post posts them), wherever `top`
    // lies: at or below the latency switch the throughput launches run down to `top` and the latency phase has nothing left.
    MailArgs mail = mail_in;
    if (stop != 0 || mail.top >= log_m) mail.top = 0;
    const uint32_t end = stop == 0 ? mail.top : stop;
    const uint32_t latency_depth = stop + kMerkleLatencyLog > end ? stop + kMerkleLatencyLog : end;
    const uint32_t floor_depth = throughput_only ? tp_floor : latency_depth;
    while (depth > floor_depth) {
        uint32_t k = depth - floor_depth;
        if (k > merkle_max_k()) k = merkle_max_k();
        size_t lanes = (size_t)1 << (depth - stop - k);         // >= 2^17: a multiple of the block size
        uint32_t blocks = (uint32_t)(lanes / kMerkleThreads);
        size_t sh = (size_t)(kMerkleThreads / 64) * (k + 1) * 128 * sizeof(uint4);
        ScopedKernelTimer tm(prof, leaf ? K_MERKLE_LEAF : K_MERKLE_INNER, first_bytes(merkle_bytes(leaf, depth - stop, k)), s, merkle_ops(leaf, depth - stop, k, hash));
        if (hash == ZK_HASH_BLAKE2S) {
            if constexpr (B2sSrc<SRC>::ok) {
                if (leaf) hipLaunchKernelGGL((b2s_subtree_kernel<SRC, true>), dim3(blocks), dim3(kMerkleThreads), sh, s, src, nodes, depth, k, off_at(depth));
                else hipLaunchKernelGGL((b2s_subtree_kernel<PlainSrc, false>), dim3(blocks), dim3(kMerkleThreads), sh, s, none, nodes, depth, k, off_at(depth));
            }
        } else if (hash == ZK_HASH_FIELD) {
            if (leaf) hipLaunchKernelGGL((merkle_subtree_kernel<SRC, true, 1>), dim3(blocks), dim3(kMerkleThreads), sh, s, src, nodes, depth, k, off_at(depth));
            else hipLaunchKernelGGL((merkle_subtree_kernel<PlainSrc, false, 1>), dim3(blocks), dim3(kMerkleThreads), sh, s, none, nodes, depth, k, off_at(depth));
        } else {
            if (leaf) hipLaunchKernelGGL((merkle_subtree_kernel<SRC, true, 0>), dim3(blocks), dim3(kMerkleThreads), sh, s, src, nodes, depth, k, off_at(depth));
            else hipLaunchKernelGGL((merkle_subtree_kernel<PlainSrc, false, 0>), dim3(blocks), dim3(kMerkleThreads), sh, s, none, nodes, depth, k, off_at(depth));
        }
        leaf = false;
        depth -= k;
    }
    // the latency phase is skipped when the throughput launches have reached `end` (a tree of ONE leaf has had none: its leaf
    // is hashed by the launch below, as ever)
    if (throughput_only || (depth < log_m && depth <= end)) return hipGetLastError();
    auto launch_wg = [&](uint32_t j, uint32_t j2) {
        const uint32_t span = depth - stop;
        const uint32_t blocks = 1u << (span - j);
        const uint32_t lds_log = j2 && span - j > j ? span - j : j;       // the continuation holds all `blocks` nodes
        const size_t sh = ((size_t)2 << lds_log) * sizeof(uint4) + 2 * 16 * 128 * sizeof(uint32_t);
        ScopedKernelTimer tm(prof, K_MERKLE_TOP, first_bytes(merkle_bytes(leaf, span, j)) + (j2 ? merkle_bytes(false, span - j, j2) : 0.0), s,
                             merkle_ops(leaf, span, j, hash) + (j2 ? merkle_ops(false, span - j, j2, hash) : 0.0));
        if (hash == ZK_HASH_BLAKE2S) {
            if constexpr (B2sSrc<SRC>::ok) {
                if (leaf) hipLaunchKernelGGL((merkle_wg_kernel<SRC, true, 2>), dim3(blocks), dim3(kWgThreads), sh, s, src, nodes, depth, j, mail, off_at(depth), j2, lds_log);
                else hipLaunchKernelGGL((merkle_wg_kernel<PlainSrc, false, 2>), dim3(blocks), dim3(kWgThreads), sh, s, none, nodes, depth, j, mail, off_at(depth), j2, lds_log);
            }
        } else if (hash == ZK_HASH_FIELD) {
            if (leaf) hipLaunchKernelGGL((merkle_wg_kernel<SRC, true, 1>), dim3(blocks), dim3(kWgThreads), sh, s, src, nodes, depth, j, mail, off_at(depth), j2, lds_log);
            else hipLaunchKernelGGL((merkle_wg_kernel<PlainSrc, false, 1>), dim3(blocks), dim3(kWgThreads), sh, s, none, nodes, depth, j, mail, off_at(depth), j2, lds_log);
        } else {
            if (leaf) hipLaunchKernelGGL((merkle_wg_kernel<SRC, true, 0>), dim3(blocks), dim3(kWgThreads), sh, s, src, nodes, depth, j, mail, off_at(depth), j2, lds_log);
            else hipLaunchKernelGGL((merkle_wg_kernel<PlainSrc, false, 0>), dim3(blocks), dim3(kWgThreads), sh, s, none, nodes, depth, j, mail, off_at(depth), j2, lds_log);
        }
        leaf = false;
        depth -= j + j2;
    };
    // A whole tree with a counter at hand finishes in ONE launch: every workgroup reduces 2^j inputs to a node and the one
    // that finishes last carries on with those nodes (merkle_wg_kernel: continuation).  (j, j2) is the split the level
    // cost model below likes best; a lone workgroup is a bad way to hash a small tree (2^10 leaves of the field hash:
    // 142 us in one workgroup, ~50 us as 32 workgroups and a continuation).
    const bool may_continue = stop == 0 && mail.counter != nullptr && g_merkle_continuation;
    do {
        const uint32_t span = depth - stop;
        const uint32_t levels = depth - end;
        // without a continuation: the remaining levels split evenly over launches of <= kWgMaxLog levels; this launch takes jn
        const uint32_t launches = levels ? (levels + kWgMaxLog - 1) / kWgMaxLog : 1;
        const uint32_t jn = (levels + launches - 1) / launches;
        uint32_t best_j = jn, best_j2 = 0;
        if (may_continue && levels <= 2 * kWgMaxLog) {
            // cost of the plain way to depth `end` (a further launch costs the host an enqueue on the commit -> challenge -> launch
            // path; only the two-launch case is compared, deeper trees take the plain way first)
            double best = wg_phase_us(leaf, jn, jn, hash, 1u << (span - jn));
            if (launches == 2 && span - jn <= kWgMaxLog) best += kLaunchUs + wg_phase_us(false, span - jn, levels - jn, hash, 1);
            else if (launches > 1) best = 0.0;                                  // not modelled: keep the plain way
            for (uint32_t j = 1; j < levels && j <= kWgMaxLog; ++j) {
                const uint32_t j2 = levels - j;
                if (j2 > kWgMaxLog || span - j > kWgMaxLog) continue;          // the continuation keeps 2^(span - j) nodes in LDS
                const double us = wg_phase_us(leaf, j, j, hash, 1u << (span - j)) + kContinueUs + wg_phase_us(false, span - j, j2, hash, 1);
                if (us < best) { best = us; best_j = j; best_j2 = j2; }
            }
        }
        launch_wg(best_j, best_j2);
    } while (depth > end);
    return hipGetLastError();
}

hipError_t launch_merkle_build(const uint32_t* vals, uint32_t log_m, uint32_t* nodes, hipStream_t s, Profiler* prof,
                               const MailArgs& mail, int hash) {
    return merkle_build_t(PlainSrc{vals}, 4.0 * (double)((size_t)1 << log_m), log_m, nodes, s, prof, mail, hash);
}
// Tree with coset leaves over a layer of 2^log_len values (steps in 1..3, log_len > steps): one launch hashes the 2^(log_len - steps)
// leaves into the heap, the build above them is the inner-mode build every chunked tree already ends with (mailbox and hand-over
// as for every tree).  Each lane takes up to four leaves so that the loads of the next one overlap a hash.
template <int HASH>
static void coset_leaf_launch(const uint32_t* vals, uint32_t log_len, uint32_t steps, uint32_t* nodes, uint32_t blocks, hipStream_t s) {
    const dim3 g(blocks), b(kCosetThreads);
    if (steps == 1) hipLaunchKernelGGL((coset_leaf_hash_kernel<HASH, 1>), g, b, 0, s, vals, log_len, nodes);
    else if (steps == 2) hipLaunchKernelGGL((coset_leaf_hash_kernel<HASH, 2>), g, b, 0, s, vals, log_len, nodes);
    else hipLaunchKernelGGL((coset_leaf_hash_kernel<HASH, 3>), g, b, 0, s, vals, log_len, nodes);
}
hipError_t launch_merkle_build_coset(const uint32_t* vals, uint32_t log_len, uint32_t steps, uint32_t* nodes, hipStream_t s, Profiler* prof,
                                     const MailArgs& mail, int hash) {
    if (steps == 0) return launch_merkle_build(vals, log_len, nodes, s, prof, mail, hash);
    if (steps > 3 || log_len <= steps) return hipErrorInvalidValue;
    if (hash == ZK_HASH_FIELD) {
        hipError_t e = ensure_fieldhash_consts();
        if (e != hipSuccess) return e;
    }
    const uint32_t log_m = log_len - steps;
    const size_t leaves = (size_t)1 << log_m;
    const size_t lanes = leaves > 4 * (size_t)kCosetThreads ? leaves / 4 : leaves;
    const uint32_t blocks = (uint32_t)((lanes + kCosetThreads - 1) / kCosetThreads);
    {
        ScopedKernelTimer tm(prof, K_MERKLE_LEAF, 4.0 * (double)((size_t)1 << log_len) + 32.0 * (double)leaves, s,
                             (double)leaves * hash_leaf_ops(hash));
        if (hash == ZK_HASH_BLAKE2S) coset_leaf_launch<2>(vals, log_len, steps, nodes, blocks, s);
        else if (hash == ZK_HASH_FIELD) coset_leaf_launch<1>(vals, log_len, steps, nodes, blocks, s);
        else coset_leaf_launch<0>(vals, log_len, steps, nodes, blocks, s);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return merkle_build_t(PlainSrc{nullptr}, 0.0, log_m, nodes, s, prof, mail, hash, log_m, 0, false);
}
// The same over a proof-major batch of 2^log_batch layers (vals: [batch][2^log_len]): the trees of the batch are the bottom of ONE
// heap over batch * m leaves, m = 2^(log_len - steps) per proof.  Global leaf g belongs to proof p = g >> log_m and is that
// proof's leaf c = g & (m - 1): it holds vals[(p << log_len) + c + u m], u < 2^steps (the single kernel over batch * len values
// would mix the slots of different proofs), and its digest goes to heap position batch * m - 1 + g.  Everything else is
// coset_leaf_hash_kernel's: one compression per leaf, the next leaf's loads in flight during a hash, the same number of trips for
// every lane, and each of the s loads a coalesced run across the wave when m >= 64 (below that a wave spans several proofs and a
// load is one run per proof).
template <int HASH, int STEPS>
__global__ __launch_bounds__(kCosetThreads) void coset_leaf_hash_batch_kernel(const uint32_t* __restrict__ vals, uint32_t log_len, uint32_t log_batch,
                                                                              uint32_t* __restrict__ nodes) {
    constexpr int S = 1 << STEPS;
    const uint32_t log_m = log_len - STEPS;
    const size_t m = (size_t)1 << log_m;                         // leaves per proof, also the distance between two slots of a leaf
    const size_t total = m << log_batch;
    const size_t stride = (size_t)gridDim.x * kCosetThreads;     // a power of two <= total, or every leaf has a lane of its own
    size_t g = (size_t)blockIdx.x * kCosetThreads + threadIdx.x;
    if (g >= total) return;
    uint32_t v[S], nx[S] = {};
    {
        const uint32_t* src = vals + ((g >> log_m) << log_len) + (g & (m - 1));
#pragma unroll
        for (int u = 0; u < S; ++u) v[u] = src[(size_t)u * m];
    }
    bool more;
#pragma unroll 1
    do {
        const size_t gn = g + stride;
        more = gn < total;
        if (more) {
            const uint32_t* src = vals + ((gn >> log_m) << log_len) + (gn & (m - 1));
#pragma unroll
            for (int u = 0; u < S; ++u) nx[u] = src[(size_t)u * m];
        }
        store_digest(nodes, total - 1 + g, coset_leaf_digest<HASH, S>(v));
#pragma unroll
        for (int u = 0; u < S; ++u) v[u] = nx[u];
        g = gn;
    } while (more);
}
template <int HASH>
static void coset_leaf_batch_launch(const uint32_t* vals, uint32_t log_len, uint32_t steps, uint32_t log_batch, uint32_t* nodes, uint32_t blocks,
                                    hipStream_t s) {
    const dim3 g(blocks), b(kCosetThreads);
    if (steps == 1) hipLaunchKernelGGL((coset_leaf_hash_batch_kernel<HASH, 1>), g, b, 0, s, vals, log_len, log_batch, nodes);
    else if (steps == 2) hipLaunchKernelGGL((coset_leaf_hash_batch_kernel<HASH, 2>), g, b, 0, s, vals, log_len, log_batch, nodes);
    else hipLaunchKernelGGL((coset_leaf_hash_batch_kernel<HASH, 3>), g, b, 0, s, vals, log_len, log_batch, nodes);
}
hipError_t launch_merkle_build_coset_batch(const uint32_t* vals, uint32_t log_len, uint32_t steps, uint32_t log_batch, uint32_t* nodes, hipStream_t s,
                                           Profiler* prof, const MailArgs& mail, int hash) {
    if (steps < 1 || steps > 3 || log_len <= steps || log_len + log_batch > 32) return hipErrorInvalidValue;
    if (hash == ZK_HASH_BLAKE2S) return hipErrorInvalidValue;   // the batched prover has no BLAKE2s yet (zk_batch_set_hash refuses it)
    if (hash == ZK_HASH_FIELD) {
        hipError_t e = ensure_fieldhash_consts();
        if (e != hipSuccess) return e;
    }
    const uint32_t log_m = log_len - steps + log_batch;          // leaves of the batch heap
    const size_t leaves = (size_t)1 << log_m;
    const size_t lanes = leaves > 4 * (size_t)kCosetThreads ? leaves / 4 : leaves;   // up to four leaves per lane, as the single launch
    const uint32_t blocks = (uint32_t)((lanes + kCosetThreads - 1) / kCosetThreads);
    {
        ScopedKernelTimer tm(prof, K_MERKLE_LEAF, 4.0 * (double)((size_t)1 << (log_len + log_batch)) + 32.0 * (double)leaves, s,
                             (double)leaves * hash_leaf_ops(hash));
        if (hash == ZK_HASH_FIELD) coset_leaf_batch_launch<1>(vals, log_len, steps, log_batch, nodes, blocks, s);
        else coset_leaf_batch_launch<0>(vals, log_len, steps, log_batch, nodes, blocks, s);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return merkle_build_t(PlainSrc{nullptr}, 0.0, log_m, nodes, s, prof, mail, hash, log_m, 0, false);   // mail.top: the per-proof roots or below
}
// ---- row leaves of a shared proof (transcript.hpp "rows") -------------------------------------------------------
// ONE tree over the 2^log_len rows of a proof-major batch (vals: [M][2^log_len], M = 2^LB): leaf i holds vals[(p << log_len) + i],
// p < M, in statement order, and its digest goes to heap position 2^log_len - 1 + i.  The walk is coset_leaf_hash_kernel's: a lane owns
// the leaves i, i + stride, ..., every lane of a wave makes the same number of trips, and each of its M loads is one coalesced run
// across the wave.  LB <= 3: the row is a coset leaf of M slots, one compression (coset_leaf_digest).  LB >= 4: the row is streamed
// in blocks of 16 (SHA-256: one message block) or 8 values (field hash: one chunk of fieldhash_row_leaf's chain); the next block --
// of this leaf, or the first of the lane's next leaf -- is loaded before the current one is compressed, and only the chaining state
// lives across blocks: 16 + 16 (8 + 8) message words and 8 state words, no scratch, no LDS.  The block loop is not unrolled, so a
// leaf kernel holds ONE inlined data compression whatever M; the SHA-256 padding block (0x80000000, 0, .., 0, 32 M) is a constant
// message per M and its whole schedule folds at compile time (a second compression of 64 rounds without a schedule).
template <int HASH, int LB>
__global__ __launch_bounds__(kCosetThreads) void row_leaf_hash_kernel(const uint32_t* __restrict__ vals, uint32_t log_len, uint32_t* __restrict__ nodes) {
    constexpr int M = 1 << LB;
    const size_t leaves = (size_t)1 << log_len;                  // also the distance between two values of a row
    const size_t stride = (size_t)gridDim.x * kCosetThreads;     // a power of two <= leaves, or one workgroup: every lane of a wave makes the same trips
    size_t c = (size_t)blockIdx.x * kCosetThreads + threadIdx.x;
    if (c >= leaves) return;
    if constexpr (LB <= 3) {
        uint32_t v[M], nx[M] = {};
#pragma unroll
        for (int u = 0; u < M; ++u) v[u] = vals[c + (size_t)u * leaves];
        bool more;
#pragma unroll 1
        do {
            const size_t cn = c + stride;
            more = cn < leaves;
            if (more) {
#pragma unroll
                for (int u = 0; u < M; ++u) nx[u] = vals[cn + (size_t)u * leaves];
            }
            store_digest(nodes, leaves - 1 + c, coset_leaf_digest<HASH, M>(v));
#pragma unroll
            for (int u = 0; u < M; ++u) v[u] = nx[u];
            c = cn;
        } while (more);
    } else {
        constexpr int CH = HASH == ZK_HASH_FIELD ? 8 : 16;       // values per compression
        constexpr int NB = M / CH;                               // data blocks of a leaf
        uint32_t cur[CH], nx[CH] = {};
#pragma unroll
        for (int u = 0; u < CH; ++u) cur[u] = vals[c + (size_t)u * leaves];
        bool more;
#pragma unroll 1
        do {
            const size_t cn = c + stride;
            more = cn < leaves;
            Digest d;
#pragma unroll
            for (int i = 0; i < 8; ++i) d.w[i] = HASH == ZK_HASH_FIELD ? 0u : SHA_IV[i];
#pragma unroll 1
            for (int k = 0; k < NB; ++k) {
                const bool last = k + 1 == NB;
                if (!last || more) {                             // block k + 1 of this leaf, or block 0 of the next one
                    const uint32_t* src = last ? vals + cn : vals + c + (size_t)(k + 1) * CH * leaves;
#pragma unroll
                    for (int u = 0; u < CH; ++u) nx[u] = src[(size_t)u * leaves];
                }
                if constexpr (HASH == ZK_HASH_FIELD) {
                    uint32_t in[kFhT];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        in[i] = k == 0 ? cur[i] : d.w[i];
                        in[8 + i] = k == 0 ? (i == 7 ? (uint32_t)M : 0u) : cur[i];
                    }
                    fh64_compress(in, d.w, g_fh_consts64);
                } else {
                    sha256_compress(d.w, cur);
                }
#pragma unroll
                for (int u = 0; u < CH; ++u) cur[u] = nx[u];
            }
            if constexpr (HASH != ZK_HASH_FIELD) {
                uint32_t pad[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 32u * M};
                sha256_compress(d.w, pad);
            }
            store_digest(nodes, leaves - 1 + c, d);
            c = cn;
        } while (more);
    }
}
template <int HASH>
static void row_leaf_launch(const uint32_t* vals, uint32_t log_len, uint32_t log_batch, uint32_t* nodes, uint32_t blocks, hipStream_t s) {
    const dim3 g(blocks), b(kCosetThreads);
    switch (log_batch) {
        case 1: hipLaunchKernelGGL((row_leaf_hash_kernel<HASH, 1>), g, b, 0, s, vals, log_len, nodes); break;
        case 2: hipLaunchKernelGGL((row_leaf_hash_kernel<HASH, 2>), g, b, 0, s, vals, log_len, nodes); break;
        case 3: hipLaunchKernelGGL((row_leaf_hash_kernel<HASH, 3>), g, b, 0, s, vals, log_len, nodes); break;
        case 4: hipLaunchKernelGGL((row_leaf_hash_kernel<HASH, 4>), g, b, 0, s, vals, log_len, nodes); break;
        case 5: hipLaunchKernelGGL((row_leaf_hash_kernel<HASH, 5>), g, b, 0, s, vals, log_len, nodes); break;
        case 6: hipLaunchKernelGGL((row_leaf_hash_kernel<HASH, 6>), g, b, 0, s, vals, log_len, nodes); break;
        case 7: hipLaunchKernelGGL((row_leaf_hash_kernel<HASH, 7>), g, b, 0, s, vals, log_len, nodes); break;
        default: hipLaunchKernelGGL((row_leaf_hash_kernel<HASH, 8>), g, b, 0, s, vals, log_len, nodes); break;
    }
}
// compressions of one row leaf of 2^log_batch values (transcript.hpp "rows")
static double row_leaf_compressions(uint32_t log_batch, int hash) {
    if (log_batch <= 3) return 1.0;
    return hash == ZK_HASH_FIELD ? (double)(1u << (log_batch - 3)) : (double)((1u << (log_batch - 4)) + 1u);
}
hipError_t launch_merkle_build_rows(const uint32_t* vals, uint32_t log_len, uint32_t log_batch, uint32_t* nodes, hipStream_t s, Profiler* prof,
                                    const MailArgs& mail, int hash) {
    if (log_batch < 1 || log_batch > 8 || log_len < 1 || log_len + log_batch > 32) return hipErrorInvalidValue;
    if (hash != ZK_HASH_SHA256 && hash != ZK_HASH_FIELD) return hipErrorInvalidValue;   // no BLAKE2s row leaf (transcript.hpp "rows")
    if (hash == ZK_HASH_FIELD) {
        hipError_t e = ensure_fieldhash_consts();
        if (e != hipSuccess) return e;
    }
    const size_t leaves = (size_t)1 << log_len;
    const size_t lanes = leaves > 4 * (size_t)kCosetThreads ? leaves / 4 : leaves;   // up to four leaves per lane, as the coset launches
    const uint32_t blocks = (uint32_t)((lanes + kCosetThreads - 1) / kCosetThreads);
    {
        ScopedKernelTimer tm(prof, K_MERKLE_LEAF, 4.0 * (double)((size_t)1 << (log_len + log_batch)) + 32.0 * (double)leaves, s,
                             (double)leaves * row_leaf_compressions(log_batch, hash) * hash_leaf_ops(hash));
        if (hash == ZK_HASH_FIELD) row_leaf_launch<1>(vals, log_len, log_batch, nodes, blocks, s);
        else row_leaf_launch<0>(vals, log_len, log_batch, nodes, blocks, s);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return merkle_build_t(PlainSrc{nullptr}, 0.0, log_len, nodes, s, prof, mail, hash, log_len, 0, false);
}
// ---- coset leaves over a batch of layers of E (launch_merkle_build_coset_ext_batch) --------------------------------
// vals: two planes [batch][2^log_len].  Global leaf g = (p, c) as in coset_leaf_hash_batch_kernel; it holds the M = 2 S words
// vals[plane * batch * len + (p << log_len) + c + u m], u < S, plane 0's first: the row leaf of M values that row_leaf_hash_kernel<HASH, STEPS + 1>
// hashes over the [M][m] array one proof's two planes are, so the digest is the one-call prover's.  M <= 8: one compression
// (coset_leaf_digest).  M = 16 (STEPS = 3): SHA-256 takes the 16 words as one message block and then the constant padding block, whose
// schedule folds at compile time; the field hash its chain of two compressions of 8 values, in a loop that is not unrolled so that the
// kernel holds one inlined permutation.  The walk, the prefetch of the lane's next leaf and the equal trip counts are the base kernel's.
template <int HASH, int M>
__device__ __forceinline__ Digest ext_leaf_digest(const uint32_t (&v)[M]) {
    if constexpr (M <= 8) {
        return coset_leaf_digest<HASH, M>(v);
    } else {
        static_assert(M == 16, "a leaf of E holds at most 2 * 8 words");
        Digest d;
        if constexpr (HASH == ZK_HASH_FIELD) {
#pragma unroll
            for (int i = 0; i < 8; ++i) d.w[i] = 0u;
#pragma unroll 1
            for (int k = 0; k < 2; ++k) {
                uint32_t in[kFhT];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    in[i] = k == 0 ? v[i] : d.w[i];
                    in[8 + i] = k == 0 ? (i == 7 ? (uint32_t)M : 0u) : v[8 + i];
                }
                fh64_compress(in, d.w, g_fh_consts64);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) d.w[i] = SHA_IV[i];
            uint32_t w[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) w[i] = v[i];
            sha256_compress(d.w, w);
            uint32_t pad[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 32u * M};
            sha256_compress(d.w, pad);
        }
        return d;
    }
}
template <int HASH, int STEPS>
__global__ __launch_bounds__(kCosetThreads) void coset_ext_leaf_hash_batch_kernel(const uint32_t* __restrict__ vals, uint32_t log_len, uint32_t log_batch,
                                                                                  uint32_t* __restrict__ nodes) {
    constexpr int S = 1 << STEPS, M = 2 * S;
    const uint32_t log_m = log_len - STEPS;
    const size_t m = (size_t)1 << log_m;                         // leaves per proof, also the distance between two slots of a leaf
    const size_t total = m << log_batch;
    const size_t plane = (size_t)1 << (log_len + log_batch);     // words of one plane
    const size_t stride = (size_t)gridDim.x * kCosetThreads;     // a power of two <= total, or every leaf has a lane of its own
    size_t g = (size_t)blockIdx.x * kCosetThreads + threadIdx.x;
    if (g >= total) return;
    uint32_t v[M], nx[M] = {};
    {
        const uint32_t* src = vals + ((g >> log_m) << log_len) + (g & (m - 1));
#pragma unroll
        for (int u = 0; u < S; ++u) { v[u] = src[(size_t)u * m]; v[S + u] = src[plane + (size_t)u * m]; }
    }
    bool more;
#pragma unroll 1
    do {
        const size_t gn = g + stride;
        more = gn < total;
        if (more) {
            const uint32_t* src = vals + ((gn >> log_m) << log_len) + (gn & (m - 1));
#pragma unroll
            for (int u = 0; u < S; ++u) { nx[u] = src[(size_t)u * m]; nx[S + u] = src[plane + (size_t)u * m]; }
        }
        store_digest(nodes, total - 1 + g, ext_leaf_digest<HASH, M>(v));
#pragma unroll
        for (int u = 0; u < M; ++u) v[u] = nx[u];
        g = gn;
    } while (more);
}
template <int HASH>
static void coset_ext_leaf_batch_launch(const uint32_t* vals, uint32_t log_len, uint32_t steps, uint32_t log_batch, uint32_t* nodes, uint32_t blocks,
                                        hipStream_t s) {
    const dim3 g(blocks), b(kCosetThreads);
    if (steps == 1) hipLaunchKernelGGL((coset_ext_leaf_hash_batch_kernel<HASH, 1>), g, b, 0, s, vals, log_len, log_batch, nodes);
    else if (steps == 2) hipLaunchKernelGGL((coset_ext_leaf_hash_batch_kernel<HASH, 2>), g, b, 0, s, vals, log_len, log_batch, nodes);
    else hipLaunchKernelGGL((coset_ext_leaf_hash_batch_kernel<HASH, 3>), g, b, 0, s, vals, log_len, log_batch, nodes);
}
hipError_t launch_merkle_build_coset_ext_batch(const uint32_t* vals, uint32_t log_len, uint32_t steps, uint32_t log_batch, uint32_t* nodes, hipStream_t s,
                                               Profiler* prof, const MailArgs& mail, int hash) {
    if (steps < 1 || steps > 3 || log_len <= steps || log_len + log_batch > 31) return hipErrorInvalidValue;
    if (hash != ZK_HASH_SHA256 && hash != ZK_HASH_FIELD) return hipErrorInvalidValue;   // a leaf of E is a row leaf: no BLAKE2s (transcript.hpp "ext")
    if (hash == ZK_HASH_FIELD) {
        hipError_t e = ensure_fieldhash_consts();
        if (e != hipSuccess) return e;
    }
    const uint32_t log_m = log_len - steps + log_batch;          // leaves of the batch heap
    const size_t leaves = (size_t)1 << log_m;
    const size_t lanes = leaves > 4 * (size_t)kCosetThreads ? leaves / 4 : leaves;   // up to four leaves per lane, as the base launch
    const uint32_t blocks = (uint32_t)((lanes + kCosetThreads - 1) / kCosetThreads);
    {
        ScopedKernelTimer tm(prof, K_MERKLE_LEAF, 8.0 * (double)((size_t)1 << (log_len + log_batch)) + 32.0 * (double)leaves, s,
                             (double)leaves * row_leaf_compressions(steps + 1, hash) * hash_leaf_ops(hash));
        if (hash == ZK_HASH_FIELD) coset_ext_leaf_batch_launch<1>(vals, log_len, steps, log_batch, nodes, blocks, s);
        else coset_ext_leaf_batch_launch<0>(vals, log_len, steps, log_batch, nodes, blocks, s);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return merkle_build_t(PlainSrc{nullptr}, 0.0, log_m, nodes, s, prof, mail, hash, log_m, 0, false);   // mail.top: the per-proof roots or below
}
// commitment of a block whose leaves are still in all-to-all order (no interleave pass, no block buffer)
hipError_t launch_merkle_build_interleaved(const uint32_t* recv, uint32_t log_parts, uint32_t log_cnt, uint32_t* nodes, hipStream_t s,
                                           Profiler* prof, int hash, const MailArgs& mail) {
    uint32_t log_m = log_parts + log_cnt;
    return merkle_build_t(InterleaveSrc{recv, log_parts, log_cnt}, 4.0 * (double)((size_t)1 << log_m), log_m, nodes, s, prof, mail, hash);
}
// One chunk (1 / 2^log_chunks of the leaves, still in all-to-all order in its own receive buffer) of a
// tree over 2^log_m leaves: levels up to the chunk root.  launch_merkle_finish joins the chunk roots.
// Depth at which chunk builds hand over to launch_merkle_finish.  A chunk build is ONE leaf launch (the leaves of the
// chunk and k <= 4 levels, straight from its receive buffer: that is the part worth overlapping with the exchange of the
// next chunk); everything above -- further throughput launches and the latency phase -- runs once over the whole tree,
// at full width.  (Round 2 let every chunk run its own inner launches down to the latency switch: four quarter-width
// launches per level group, each a quarter-filled chip.)  Trees too small for that hand over at the chunk roots.
// A chunk build takes k = 3 levels, not 4: a chunk of 2^22 leaves is then 2 048 workgroups of 32 KiB of LDS (1.6 rounds
// of five per CU) instead of 1 024 of 40 KiB that start and end together, so LDS frees up all through the launch and the
// workgroups of the exchange kernel that runs beside it (rcclGenericKernel: 64 x 256 threads, 19.5 KiB of LDS each,
// measured) find room on the CUs.  The hashing rate does not depend on k (profiles/r03_ab_max_k.txt).
static constexpr uint32_t merkle_chunk_k() { return ZK_MERKLE_CHUNK_K; }
static uint32_t chunk_handover_depth(uint32_t log_m, uint32_t log_chunks) {
    const uint32_t lat = merkle_latency_log();
    if (!(log_m > lat && lat >= log_chunks + 8)) return log_chunks;
    uint32_t k = log_m - lat < merkle_max_k() ? log_m - lat : merkle_max_k();
    if (k > merkle_chunk_k()) k = merkle_chunk_k();
    return log_m - k;
}
uint32_t merkle_finish_start_depth(uint32_t log_m, uint32_t log_chunks) { return chunk_handover_depth(log_m, log_chunks); }
hipError_t launch_merkle_build_chunk(const uint32_t* recv, uint32_t log_parts, uint32_t log_cnt, uint32_t* nodes, uint32_t log_m,
                                     uint32_t chunk, hipStream_t s, Profiler* prof, int hash) {
    uint32_t log_sub = log_parts + log_cnt;
    const uint32_t h = chunk_handover_depth(log_m, log_m - log_sub);
    return merkle_build_t(InterleaveSrc{recv, log_parts, log_cnt}, 4.0 * (double)((size_t)1 << log_sub), log_m, nodes, s, prof, MailArgs{}, hash,
                          log_sub, chunk, true, h != log_m - log_sub ? h : 0u);
}
// After every chunk of a 2^log_m-leaf tree (2^log_chunks chunks) has been built down to the hand-over depth:
// the remaining throughput levels and the latency phase of the whole tree, once.
hipError_t launch_merkle_finish(uint32_t* nodes, uint32_t log_m, uint32_t log_chunks, hipStream_t s, Profiler* prof, int hash,
                                const MailArgs& mail) {
    const uint32_t start = chunk_handover_depth(log_m, log_chunks);   // depth the chunk builds stopped at
    if (start == 0) return hipSuccess;
    // the nodes at depth `start` exist: inner mode over a "tree" of 2^start inputs shares the top of the heap
    return merkle_build_t(PlainSrc{nullptr}, 0.0, start, nodes, s, prof, mail, hash, start, 0, false);
}
// fold + commit of the folded layer (a.out receives it): one pass
hipError_t launch_fold_merkle(const FoldArgs& a, uint32_t* nodes, hipStream_t s, Profiler* prof, const MailArgs& mail, int hash) {
    uint32_t log_out = a.log_m - 1;
    return merkle_build_t(FoldSrc{a}, 12.0 * (double)((size_t)1 << log_out), log_out, nodes, s, prof, mail, hash);
}
// composition + commit of cp layer 0 (a.cp receives it): one pass
hipError_t launch_compose_merkle(const ComposeArgs& a, uint32_t* nodes, hipStream_t s, Profiler* prof, const MailArgs& mail, int hash) {
    return merkle_build_t(ComposeSrc{a}, 8.0 * (double)((size_t)1 << a.logN), a.logN, nodes, s, prof, mail, hash);
}

// composition over one rank's block of a sharded proof + the subtree over it: reads the block of f (4 bytes per leaf; the
// taps hit the same lines), the range table (4), writes nothing but the tree
hipError_t launch_compose_block_merkle(const ComposeBlockArgs& b, uint32_t* nodes, hipStream_t s, Profiler* prof, const MailArgs& mail, int hash) {
    return merkle_build_t(ComposeBlockSrc{b}, 8.0 * (double)((size_t)1 << b.log_m), b.log_m, nodes, s, prof, mail, hash);
}

hipError_t launch_compose_merkle_batch(const ComposeBatchArgs& a, uint32_t log_batch, uint32_t* nodes, hipStream_t s, Profiler* prof,
                                       const MailArgs& mail, int hash) {
    uint32_t log_m = a.a.logN + log_batch;
    return merkle_build_t(ComposeBatchSrc{a.a, a.chal}, 8.0 * (double)((size_t)1 << log_m), log_m, nodes, s, prof, mail, hash);
}
hipError_t launch_fold_merkle_batch(const FoldBatchArgs& a, uint32_t log_batch, uint32_t* nodes, hipStream_t s, Profiler* prof,
                                    const MailArgs& mail, int hash) {
    uint32_t log_out = a.a.log_m - 1 + log_batch;
    return merkle_build_t(FoldBatchSrc{a.a, a.chal}, 12.0 * (double)((size_t)1 << log_out), log_out, nodes, s, prof, mail, hash);
}

// Copies host-built pieces (tree tops, small layers) from the mapped staging buffer into the device
// arrays so that the device state is complete after a proof (zk_merkle_path, zk_layer_read).
__global__ __launch_bounds__(1024) void scatter_kernel(const uint32_t* stage, const ScatterSeg* segs, uint32_t* trees, uint32_t* layers) {
    const ScatterSeg sg = segs[blockIdx.x];
    uint32_t* dst = (sg.kind ? layers : trees) + sg.dst;
    const uint32_t* src = stage + sg.src;
    if (((sg.src | sg.dst | sg.words) & 3) == 0) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (uint32_t i = threadIdx.x; i < sg.words / 4; i += blockDim.x) d4[i] = s4[i];
    } else {
        for (uint32_t i = threadIdx.x; i < sg.words; i += blockDim.x) dst[i] = src[i];
    }
}
hipError_t launch_scatter(const uint32_t* stage, const ScatterSeg* segs, uint32_t count, double words, uint32_t* trees, uint32_t* layers,
                          hipStream_t s, Profiler* prof) {
    if (!count) return hipSuccess;
    ScopedKernelTimer tm(prof, K_GATHER, 8.0 * words, s);
    hipLaunchKernelGGL(scatter_kernel, dim3(count), dim3(1024), 0, s, stage, segs, trees, layers);
    return hipGetLastError();
}

// ===========================================================================
// Roofline probe of the Merkle kernels (measurement only; bench.py: roofline.valu.chain_*)
// ===========================================================================
// Every lane runs a chain of `hashes` inner hashes d <- H(d, d ^ seed) (merkle.rs:42-45 shape), no memory traffic:
// the rate at which the COMPILED hash issues, which is what the subtree kernels can reach at best at the same
// residency.  Each wave records its lifetime in shader clocks and in the 100 MHz constant clock (the clock held).
template <int HASH>
__global__ __launch_bounds__(256) void hash_chain_probe_kernel(uint32_t* out, uint32_t seed, uint32_t hashes, unsigned long long* rec) {
    Digest d;
#pragma unroll
    for (int i = 0; i < 8; ++i) d.w[i] = (seed * (uint32_t)(i + 1) + threadIdx.x + blockIdx.x * 977u) % P;
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#pragma unroll 1
    for (uint32_t it = 0; it < hashes; ++it) {
        Digest r = d;
        r.w[0] ^= seed;
        if (HASH == ZK_HASH_FIELD) r.w[0] &= 0x7fffffffu;   // stays a canonical residue
        d = Hasher<HASH>::inner(d, r);
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) x ^= d.w[i];
    out[blockIdx.x * 256 + threadIdx.x] = x;
    if (rec && (threadIdx.x & 63) == 0) {
        rec[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2] = c1 - c0;
        rec[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + 1] = r1 - r0;
    }
}
hipError_t launch_hash_chain_probe(int hash, uint32_t blocks, uint32_t* out, uint32_t seed, uint32_t hashes, unsigned long long* rec, hipStream_t s) {
    if (hash == ZK_HASH_BLAKE2S) {
        hipLaunchKernelGGL(hash_chain_probe_kernel<2>, dim3(blocks), dim3(256), 0, s, out, seed, hashes, rec);
    } else if (hash == ZK_HASH_FIELD) {
        hipError_t e = ensure_fieldhash_consts();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(hash_chain_probe_kernel<1>, dim3(blocks), dim3(256), 0, s, out, seed, hashes, rec);
    } else {
        hipLaunchKernelGGL(hash_chain_probe_kernel<0>, dim3(blocks), dim3(256), 0, s, out, seed, hashes, rec);
    }
    return hipGetLastError();
}

// The three forms of the field hash on the device against each other (test hook: zk_probe_fieldhash_forms).  Thread t hashes a
// pseudo-random pair of digests and a leaf value, every 16th thread one of the edge patterns (words 0, P - 1, all P - 1, all 0,
// raw words >= P): double precision (what every tree is built with) and 32-bit Montgomery (the host's form) must agree word for
// word and be canonical; the 16-lane row form of the narrow levels is compared on the first pair of each row.
__global__ __launch_bounds__(256) void fieldhash_forms_kernel(uint32_t seed, uint32_t* bad, uint32_t* first_bad) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t x = (t + 1u) * 2654435761u + seed;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    Digest l, r;
#pragma unroll
    for (int i = 0; i < 8; ++i) { l.w[i] = rnd() % P; r.w[i] = rnd() % P; }
    if ((t & 15u) == 1) { l.w[t & 7u] = 0; r.w[(t >> 4) & 7u] = P - 1; }
    if ((t & 15u) == 2) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { l.w[i] = P - 1; r.w[i] = P - 1; }
    }
    if ((t & 15u) == 3) { l.w[0] = 0xFFFFFFFFu; r.w[7] = P; r.w[3] = P + 5; }                  // raw words >= P (field.rs:20-24)
    if ((t & 15u) == 4) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { l.w[i] = 0; r.w[i] = 0; }
    }
    uint32_t v = rnd();
    if ((t & 7u) == 0) v = (t & 8u) ? 0xFFFFFFFFu : P - 1;
    if (t == 5) v = 0;
    const Digest a = fieldhash_inner(l, r, g_fh_consts), b = fieldhash_inner64(l, r, g_fh_consts64);
    const Digest c = fieldhash_leaf(v, g_fh_consts), d = fieldhash_leaf64(v, g_fh_consts64);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) ok = ok && a.w[i] == b.w[i] && c.w[i] == d.w[i] && b.w[i] < P && d.w[i] < P;
    // row form: the 16 lanes of a row hash the pair of the row's first thread
    const uint32_t g = threadIdx.x & 15u;
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t lw = __shfl(l.w[i], (int)(threadIdx.x & ~15u) & 63, 64), rw = __shfl(r.w[i], (int)(threadIdx.x & ~15u) & 63, 64);
        if (g == (uint32_t)i) word = lw;
        if (g == (uint32_t)i + 8u) word = rw;
    }
    {   // quad form: the 4 lanes of a quad hash the pair of the quad's first thread
        const uint32_t q4 = threadIdx.x & 3u;
        const int src = (int)(threadIdx.x & ~3u) & 63;
        uint32_t in4[4], out4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t wsel = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint32_t lw = __shfl(l.w[i], src, 64), rw = __shfl(r.w[i], src, 64);
                if ((int)(4 * q4) + j == i) wsel = lw;
                if ((int)(4 * q4) + j == i + 8) wsel = rw;
            }
            in4[j] = wsel;
        }
        fieldhash_inner_quad_f64(in4, q4, out4, g_fh_consts64);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t want = __shfl(b.w[i], src, 64);
            if (q4 < 2 && (int)(4 * q4) <= i && i < (int)(4 * q4) + 4 && out4[i - 4 * (int)q4 < 0 ? 0 : (i - 4 * (int)q4) & 3] != want) ok = false;
        }
    }
    const uint32_t row = fieldhash_inner_row16(word, g, g_fh_consts), row64 = fieldhash_inner_row16_f64(word, g, g_fh_consts64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t want = __shfl(b.w[i], (int)(threadIdx.x & ~15u) & 63, 64);
        if (g == (uint32_t)i && (row != want || row64 != want)) ok = false;
    }
    {   // Directed inputs of the double-precision S-box (fieldhash_f64.hpp: the s_0 path of the partial rounds squares up to 2^41.9,
        // where the quotient of the first product needs all 53 bits): integers of magnitude 2^37.8 ... 2^42 and multiples of P next to
        // them, both signs, against x^5 (mod P) in plain integer arithmetic.
        const double mags[6] = {236118324143.0 /* 2^37.78 */, 3829546563953.0 /* 2^41.8 */, 4104397301943.0 /* 2^41.9 */, 4398046511103.0 /* 2^42 - 1 */,
                                (double)P * 1365.0, (double)P * 1024.0};
        const uint32_t k = t % 6u;
        double xd = mags[k] + (double)(int)((rnd() & 0xFFFFu)) - 32768.0 + (k >= 4 ? (double)(rnd() % 3u) - 1.0 : 0.0);
        if (t & 8u) xd = -xd;
        const long long xi = (long long)xd;                           // exact: |x| < 2^43
        const uint64_t res = (uint64_t)(((xi % (long long)P) + (long long)P) % (long long)P);
        const uint64_t x2 = res * res % P, x4 = x2 * x2 % P, want5 = x4 * res % P;
        if (fh64_canonical(fh64_sbox(xd)) != (uint32_t)want5) ok = false;
        // and a whole partial round from a state whose s_0 sits at that magnitude: every output against integer arithmetic
        double st[kFhT];
        uint64_t ref[kFhT];
#pragma unroll
        for (int i = 0; i < kFhT; ++i) { st[i] = i ? (double)(l.w[i & 7] >> 1) - (double)(r.w[i & 7] >> 2) : xd; }
#pragma unroll
        for (int i = 0; i < kFhT; ++i) { const long long v = (long long)st[i]; ref[i] = (uint64_t)(((v % (long long)P) + (long long)P) % (long long)P); }
        const double rc = g_fh_consts64.rc_part[t % kFhRP];
        fh64_partial_round<true>(st, rc);
        {
            const uint64_t y = (ref[0] + (uint64_t)rc) % P, y2 = y * y % P, y4 = y2 * y2 % P;
            ref[0] = y4 * y % P;
            uint64_t sum = 0;
#pragma unroll
            for (int i = 0; i < kFhT; ++i) sum = (sum + ref[i]) % P;
            uint64_t outw[kFhT];
            outw[0] = (sum + 2 * (P - ref[0])) % P;                   // d_0 = -2
#pragma unroll
            for (int i = 1; i < kFhT; ++i) outw[i] = (((uint64_t)1 << (i - 1)) % P * ref[i] + sum) % P;
#pragma unroll
            for (int i = 0; i < kFhT; ++i)
                if (fh64_canonical(st[i]) != (uint32_t)outw[i]) ok = false;
        }
    }
    if (!ok) { atomicAdd(bad, 1u); atomicMin(first_bad, t); }
}
hipError_t launch_fieldhash_forms(uint32_t blocks, uint32_t seed, uint32_t* d_res, hipStream_t s) {
    hipError_t e = ensure_fieldhash_consts();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fieldhash_forms_kernel, dim3(blocks), dim3(256), 0, s, seed, d_res, d_res + 1);
    return hipGetLastError();
}

// ===========================================================================
// Trace generation for batches
// ===========================================================================
// prover.rs:32-39 is a serial recurrence, so one trace cannot be parallelised; many independent
// traces can.  One lane per trace: out[t*count + i] = a_i of trace t (a0[t], a1[t] seeds).
__global__ __launch_bounds__(64) void trace_fibsq_batch_kernel(const uint32_t* a0, const uint32_t* a1, uint32_t batch,
                                                               uint32_t count, uint32_t* out, uint32_t stride) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= batch) return;
    uint32_t* row = out + (size_t)t * stride;
    // Montgomery domain: squares of Montgomery values stay Montgomery
    uint32_t x = mont_mul(a0[t], R2_MONT), y = mont_mul(a1[t], R2_MONT);
    if (count > 0) row[0] = mont_mul(x, 1u);
    if (count > 1) row[1] = mont_mul(y, 1u);
    for (uint32_t i = 2; i < count; ++i) {
        uint32_t z = add(mont_mul(x, x), mont_mul(y, y));
        row[i] = mont_mul(z, 1u);
        x = y; y = z;
    }
}

hipError_t launch_trace_fibsq_batch(const uint32_t* a0, const uint32_t* a1, uint32_t batch, uint32_t count, uint32_t* out, hipStream_t s,
                                    uint32_t stride) {
    if (!batch) return hipSuccess;
    hipLaunchKernelGGL(trace_fibsq_batch_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, a0, a1, batch, count, out, stride ? stride : count);
    return hipGetLastError();
}

// ===========================================================================
// Interleave (cyclic <-> block layout change around the multi-GPU exchange)
// ===========================================================================
// in: 2^log_parts pieces of 2^log_cnt words; out[u * parts + q] = in[q * cnt + u]
__global__ void interleave_kernel(const uint32_t* in, uint32_t* out, uint32_t log_parts, uint32_t log_cnt) {
    size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= ((size_t)1 << (log_parts + log_cnt))) return;
    size_t q = o & (((size_t)1 << log_parts) - 1), u = o >> log_parts;
    out[o] = in[(q << log_cnt) + u];
}

__global__ __launch_bounds__(256) void halo_pack_kernel(const uint32_t* loc, uint32_t* out, uint32_t log_per, uint32_t lg, uint32_t h) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (h << lg)) return;
    const uint32_t q = i / h, u = i - q * h;
    const size_t mask = ((size_t)1 << (log_per + lg)) - 1;
    out[i] = loc[((((size_t)q + 1) << log_per) + u) & mask];
}
hipError_t launch_halo_pack(const uint32_t* loc, uint32_t* out, uint32_t log_per, uint32_t lg, uint32_t h, hipStream_t s) {
    const uint32_t total = h << lg;
    hipLaunchKernelGGL(halo_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, s, loc, out, log_per, lg, h);
    return hipGetLastError();
}
hipError_t launch_interleave(const uint32_t* in, uint32_t* out, uint32_t log_parts, uint32_t log_cnt, hipStream_t s) {
    size_t total = (size_t)1 << (log_parts + log_cnt);
    uint32_t blocks = (uint32_t)((total + 255) / 256);
    hipLaunchKernelGGL(interleave_kernel, dim3(blocks), dim3(256), 0, s, in, out, log_parts, log_cnt);
    return hipGetLastError();
}

// ---- known-pattern exchange (self-test of the sharded prover's transport, shard.hip) ----------------------------
__global__ void pattern_fill_kernel(uint32_t* dst, uint32_t rank, uint32_t log_per, uint32_t log_parts) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ((size_t)1 << (log_per + log_parts))) return;
    dst[i] = shard_pattern(rank, (uint32_t)(i >> log_per), (uint32_t)(i & (((size_t)1 << log_per) - 1)));
}
__global__ void pattern_check_kernel(const uint32_t* src, uint32_t rank, uint32_t log_per, uint32_t log_parts, uint32_t log_chunks, uint32_t* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ((size_t)1 << (log_per + log_parts))) return;
    const uint32_t log_cc = log_per - log_chunks;
    const uint32_t u = (uint32_t)(i & (((size_t)1 << log_cc) - 1));
    const uint32_t q = (uint32_t)(i >> log_cc) & ((1u << log_parts) - 1u), c = (uint32_t)(i >> (log_cc + log_parts));
    if (src[i] != shard_pattern(q, rank, (c << log_cc) | u)) {
        atomicAdd(&out[0], 1u);
        atomicMin(&out[1], (uint32_t)i);
    }
}
hipError_t launch_pattern_fill(uint32_t* dst, uint32_t rank, uint32_t log_per, uint32_t log_parts, hipStream_t s) {
    const size_t total = (size_t)1 << (log_per + log_parts);
    hipLaunchKernelGGL(pattern_fill_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, dst, rank, log_per, log_parts);
    return hipGetLastError();
}
hipError_t launch_pattern_check(const uint32_t* src, uint32_t rank, uint32_t log_per, uint32_t log_parts, uint32_t log_chunks, uint32_t* out, hipStream_t s) {
    const size_t total = (size_t)1 << (log_per + log_parts);
    hipLaunchKernelGGL(pattern_check_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, src, rank, log_per, log_parts, log_chunks, out);
    return hipGetLastError();
}

// ===========================================================================
// Decommit gather
// ===========================================================================
__global__ void gather_kernel(const uint32_t* src, const uint64_t* offsets, uint32_t count, uint32_t words, uint32_t* out) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= count * words) return;
    uint32_t item = idx / words, w = idx % words;
    out[idx] = src[offsets[item] + w];
}

hipError_t launch_gather(const uint32_t* src, const uint64_t* offsets, uint32_t count, uint32_t words,
                         uint32_t* out, hipStream_t s, Profiler* prof) {
    if (!count) return hipSuccess;
    ScopedKernelTimer tm(prof, K_GATHER, 8.0 * (double)count * words, s);
    uint32_t total = count * words, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(gather_kernel, dim3(blocks), dim3(256), 0, s, src, offsets, count, words, out);
    return hipGetLastError();
}


// One launch for a whole decommitment: work list and results in host-mapped memory, flag behind the results.
constexpr int kFetchThreads = 1024;
__global__ __launch_bounds__(kFetchThreads) void fetch_kernel(const uint32_t* layers, const uint32_t* trees, const uint64_t* items, uint32_t nv,
                                                              uint32_t ndg, uint32_t* out, uint32_t* mailbox, uint32_t seq, uint32_t* counter) {
    const uint32_t stride = gridDim.x * kFetchThreads;
    for (uint32_t idx = blockIdx.x * kFetchThreads + threadIdx.x; idx < 2 * ndg + nv; idx += stride) {
        if (idx < 2 * ndg) {                                      // half a node per thread: 16-byte accesses on both sides
            const uint4* src = reinterpret_cast<const uint4*>(trees + items[nv + (idx >> 1)]);
            reinterpret_cast<uint4*>(out)[idx] = src[idx & 1u];
        } else {
            const uint32_t i = idx - 2 * ndg;
            out[8 * (size_t)ndg + i] = layers[items[i]];
        }
    }
    __threadfence_system();                                       // this thread's results are in host memory ...
    __syncthreads();
    if (threadIdx.x == 0) {
        bool last = true;
        if (gridDim.x > 1) {                                      // ... and so are everybody else's
            last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
            if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (last) __hip_atomic_store(&mailbox[0], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t launch_fetch(const uint32_t* layers, const uint32_t* trees, const uint64_t* items, uint32_t nv, uint32_t ndg, uint32_t* out,
                        uint32_t* mailbox, uint32_t seq, uint32_t* counter, hipStream_t s, Profiler* prof) {
    ScopedKernelTimer tm(prof, K_GATHER, 8.0 * ((double)nv + 8.0 * (double)ndg), s);
    const uint32_t work = 2 * ndg + nv;
    uint32_t blocks = (work + kFetchThreads - 1) / kFetchThreads;
    if (blocks == 0) blocks = 1;
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(fetch_kernel, dim3(blocks), dim3(kFetchThreads), 0, s, layers, trees, items, nv, ndg, out, mailbox, seq, counter);
    return hipGetLastError();
}

// One whole level of a heap for the host: the 2^level_log digests of depth level_log are contiguous (nodes + (2^level_log - 1) * 8,
// 2^(level_log + 3) words) and go to host-mapped memory with 16-byte accesses on both sides; the flag follows them by fetch_kernel's
// protocol.  A launch of its own behind the build on the same stream: the kernel boundary has made every node visible, so ordinary
// loads do.  Workgroups: the link (PCIe Gen5 x16, 63 GB/s) has to be kept full of posted writes; at a round trip of a few
// microseconds that is a few hundred KiB in flight, and 64 workgroups of 256 lanes hold 256 KiB per trip -- the same width
// fetch_kernel uses at most.  More workgroups only add arrivals on the counter; a level of <= 2^9 digests takes one.
constexpr int kPostThreads = 256;
constexpr uint32_t kPostMaxBlocks = 64, kPostQuadsPerBlock = 1024;
__global__ __launch_bounds__(kPostThreads) void digest_level_post_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, uint32_t quads,
                                                                         uint32_t* flag, uint32_t seq, uint32_t* counter) {
    const uint32_t stride = gridDim.x * kPostThreads;
    for (uint32_t i = blockIdx.x * kPostThreads + threadIdx.x; i < quads; i += stride) dst[i] = src[i];
    __threadfence_system();                                       // this thread's digests are in host memory ...
    __syncthreads();
    if (threadIdx.x == 0) {
        bool last = true;
        if (gridDim.x > 1) {                                      // ... and so are everybody else's
            last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
            if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (last) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t launch_digest_level_post(const uint32_t* nodes, uint32_t level_log, uint32_t* host_digests, uint32_t* flag, uint32_t seq,
                                    uint32_t* counter, hipStream_t s, Profiler* prof) {
    if (level_log > 28 || !nodes || !host_digests || !flag || !counter) return hipErrorInvalidValue;
    const uint32_t quads = 2u << level_log;                       // two 16-byte halves per digest
    ScopedKernelTimer tm(prof, K_GATHER, 64.0 * (double)((size_t)1 << level_log), s);
    uint32_t blocks = (quads + kPostQuadsPerBlock - 1) / kPostQuadsPerBlock;
    if (blocks > kPostMaxBlocks) blocks = kPostMaxBlocks;
    // (2^level_log - 1) * 8 words is 32 (2^level_log - 1) bytes: 16-byte aligned, as the heap and the host buffer are
    hipLaunchKernelGGL(digest_level_post_kernel, dim3(blocks), dim3(kPostThreads), 0, s,
                       reinterpret_cast<const uint4*>(nodes + (((size_t)1 << level_log) - 1) * 8), reinterpret_cast<uint4*>(host_digests), quads, flag, seq,
                       counter);
    return hipGetLastError();
}

}  // namespace zk
