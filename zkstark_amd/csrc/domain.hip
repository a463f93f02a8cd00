// domain.hip -- coset evaluation domains and the transforms over them (host side): power tables, the
// transform plan, LDE / composition / fold launch sequences, and the error plumbing of the C ABI.
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <new>

#include "internal.hpp"

namespace zk {
namespace impl {

namespace {
thread_local std::string g_last_error;
}

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
const char* last_error() { return g_last_error.c_str(); }

Plan make_plan(uint32_t log_m) {
    Plan p;
    uint32_t np = (log_m + kMaxRadixLog - 1) / kMaxRadixLog;
    if (np == 0) np = 1;
    uint32_t base = log_m / np, extra = log_m % np;
    p.nd = np;
    for (uint32_t d = 0; d < np; ++d) p.bits[d] = base + (d < extra ? 1 : 0);
    return p;
}

uint32_t pick_logC(uint32_t log_total, uint32_t logR) {
    uint32_t cols = log_total - logR, cap = ntt_pass_tile_log(log_total, logR) - logR;
    return cols < cap ? cols : cap;
}

// ---- power tables --------------------------------------------------------------
int build_table(uint32_t root, uint32_t log_order, DevTable* t) {
    uint32_t lo_bits = (log_order + 1) / 2, hi_bits = log_order - lo_bits;
    std::vector<uint32_t> lo((size_t)1 << lo_bits), hi((size_t)1 << hi_bits);
    uint32_t acc = 1;
    for (size_t j = 0; j < lo.size(); ++j) { lo[j] = to_mont(acc); acc = mulmod(acc, root); }
    uint32_t step = powmod(root, (uint64_t)1 << lo_bits);
    acc = 1;
    for (size_t j = 0; j < hi.size(); ++j) { hi[j] = to_mont(acc); acc = mulmod(acc, step); }
    HIPCHK(hipMalloc(&t->lo, lo.size() * 4));
    HIPCHK(hipMalloc(&t->hi, hi.size() * 4));
    HIPCHK(hipMemcpy(t->lo, lo.data(), lo.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t->hi, hi.data(), hi.size() * 4, hipMemcpyHostToDevice));
    t->lo_bits = lo_bits;
    return ZK_OK;
}
void free_table(DevTable* t) {
    if (t->lo) (void)hipFree(t->lo);
    if (t->hi) (void)hipFree(t->hi);
    t->lo = t->hi = nullptr;
}

// Inverse transform, natural order in, digit-reversed out, optionally scaled by scale_mont.
int run_dif(const uint32_t* src, uint32_t* data, uint32_t log_m, const Plan& pl, PowTable tw_inv, uint32_t L, uint32_t scale_mont, hipStream_t s, Profiler* prof,
            uint32_t batch, size_t src_stride, size_t data_stride) {
    uint32_t inner = log_m;
    for (uint32_t d = 0; d < pl.nd; ++d) {
        inner -= pl.bits[d];
        NttPassArgs a{};
        a.batch = batch; a.src_stride = d == 0 ? src_stride : data_stride; a.dst_stride = data_stride;
        a.src = d == 0 ? src : data; a.dst = data; a.log_total = log_m;
        a.logR = pl.bits[d]; a.logS = inner; a.logC = pick_logC(log_m, a.logR); a.tile_log = ntt_pass_tile_log(log_m, a.logR);
        a.L = L; a.tw = tw_inv; a.scale_mont = (inner == 0) ? scale_mont : 0;
        HIPCHK(launch_ntt_pass(a, NTT_DIF, s, prof));
    }
    return ZK_OK;
}
// Forward transform, digit-reversed in, natural out.
int run_dit(uint32_t* data, uint32_t log_m, const Plan& pl, PowTable tw, uint32_t L, hipStream_t s) {
    uint32_t inner = 0;
    for (int d = (int)pl.nd - 1; d >= 0; --d) {
        NttPassArgs a{};
        a.src = data; a.dst = data; a.log_total = log_m;
        a.logR = pl.bits[d]; a.logS = inner; a.logC = pick_logC(log_m, a.logR); a.tile_log = ntt_pass_tile_log(log_m, a.logR);
        a.L = L; a.tw = tw;
        HIPCHK(launch_ntt_pass(a, NTT_DIT, s));
        inner += pl.bits[d];
    }
    return ZK_OK;
}



void dom_free(zk_dom* d) {
    if (!d) return;
    free_table(&d->H); free_table(&d->Hinv); free_table(&d->W);
    if (d->d_inv_xm1) (void)hipFree(d->d_inv_xm1);
    delete d;
}

// fold_only: tables for fri_fold only (no w-power table, no 1/(x-1) table)
int dom_make(int device, uint32_t log_n, uint32_t log_b, uint32_t shift, bool fold_only, hipStream_t stream, zk_dom** out) {
    *out = nullptr;
    if (log_n < 1 || log_b > 5 || log_n + log_b > 30 || log_n + log_b < 1)
        return fail(ZK_ERR_INVALID, "domain: need 1 <= log_n, log_blowup <= 5, log_n + log_blowup <= 30 (got %u, %u)", log_n, log_b);
    if (shift == 0 || shift >= P) return fail(ZK_ERR_INVALID, "domain: shift must be a non-zero canonical residue");
    HIPCHK(hipSetDevice(device));
    zk_dom* d = new (std::nothrow) zk_dom();
    if (!d) return fail(ZK_ERR_NOMEM, "out of host memory");
    d->device = device;
    d->log_n = log_n; d->log_b = log_b; d->L = log_n + log_b;
    d->n = (size_t)1 << log_n; d->B = (size_t)1 << log_b; d->N = d->n << log_b;
    d->shift = shift;
    d->g = root_of_unity(log_n);
    d->h = root_of_unity(d->L);
    d->plan = make_plan(log_n);
    int rc;
    if ((rc = build_table(d->h, d->L, &d->H)) || (rc = build_table(invmod(d->h), d->L, &d->Hinv))) { dom_free(d); return rc; }
    uint32_t gm1 = invmod(d->g);
    d->shift_mont = to_mont(shift);
    d->gm1_mont = to_mont(gm1);
    d->gm2_mont = to_mont(mulmod(gm1, gm1));
    d->gm3_mont = to_mont(mulmod(mulmod(gm1, gm1), gm1));
    d->ninv_mont = to_mont(invmod((uint32_t)(d->n % P)));
    d->inv2_mont = to_mont(invmod(2));
    {
        const uint32_t inv2 = invmod(2);
        uint32_t wr = shift;                                     // w^(2^r)
        for (uint32_t r = 0; r < d->L && r < 32; ++r) { d->fold_k[r] = mulmod(invmod(wr), inv2); wr = mulmod(wr, wr); }
        uint32_t xn = powmod(shift, d->n);                       // x^n on the domain takes B values: shift^n (h^n)^(i mod B)
        const uint32_t hn = powmod(d->h, d->n);
        for (size_t r = 0; r < d->B; ++r) { const uint32_t den = sub(xn, 1); d->inv_den[r] = den ? invmod(den) : 0u; xn = mulmod(xn, hn); }
    }
    if (!fold_only) {
        if ((rc = build_table(shift, log_n, &d->W))) { dom_free(d); return rc; }
        // x_i - 1 must be invertible on the whole domain: shift^N != 1
        if (powmod(shift, d->N) == 1) { dom_free(d); return fail(ZK_ERR_INVALID, "domain: shift lies in the evaluation subgroup"); }
        hipError_t e = hipMalloc((void**)&d->d_inv_xm1, d->N * 4);
        if (e != hipSuccess) { dom_free(d); return fail(ZK_ERR_NOMEM, "hipMalloc(%zu) failed", d->N * 4); }
        d->device_bytes += d->N * 4;
        e = launch_build_inv_xm1(d->d_inv_xm1, d->L, d->H.view(), d->shift_mont, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { dom_free(d); return fail(ZK_ERR_HIP, "inv_xm1 build failed: %s", hipGetErrorString(e)); }
    }
    *out = d;
    return ZK_OK;
}

// lagrange + solve over the coset (polynomial.rs:337, :49; prover.rs:60-70).
// d_trace: n words (a[0..n-2], 0); d_coef: 2n words scratch; d_out: N words.
// batch > 1: `batch` independent traces, proof b at d_trace + b*n, d_coef + b*2n, d_out + b*N.
int dom_lde(const zk_dom* d, const uint32_t* d_trace, uint32_t* d_coef, uint32_t* d_out, hipStream_t s, Profiler* prof, uint32_t batch) {
    const size_t ts = batch > 1 ? d->n : 0, cs = batch > 1 ? 2 * d->n : 0, os = batch > 1 ? d->N : 0;
    // iNTT_g of (a_0 .. a_{n-2}, 0): natural -> digit-reversed, unscaled (1/n is folded into the next pass)
    int rc = run_dif(d_trace, d_coef, d->log_n, d->plan, d->Hinv.view(), d->L, 0, s, prof, batch, ts, cs);
    if (rc) return rc;
    // virtual-point correction, coset shift and 1/n (coef_prepare): applied by the first LDE pass, which loads the
    // coefficient blocks of its tile once, prepares them and keeps them in LDS for the B columns that use them; only
    // shapes the register-radix kernel does not take run the separate sweep d_coef[0..n) -> d_coef[n..2n)
    uint32_t* d_prep = d_coef + d->n;
    CoefPrepArgs pa{};
    pa.log_n = d->log_n; pa.log_b = d->log_b;
    pa.tw = d->H.view(); pa.wtab = d->W.view(); pa.ninv_mont = d->ninv_mont;
    pa.nd = d->plan.nd;
    for (uint32_t t = 0; t < d->plan.nd; ++t) pa.dig_bits[t] = d->plan.bits[t];
    // size-N forward transform of the zero-padded coefficients
    uint32_t inner = d->log_b;
    for (int q = (int)d->plan.nd - 1; q >= 0; --q) {
        NttPassArgs a{};
        a.log_total = d->L; a.logR = d->plan.bits[q]; a.logS = inner; a.logC = pick_logC(d->L, a.logR); a.tile_log = ntt_pass_tile_log(d->L, a.logR);
        a.L = d->L; a.tw = d->H.view();
        a.dst = d_out;
        a.batch = batch; a.dst_stride = os; a.src_stride = os;
        if (q == (int)d->plan.nd - 1) {
            if (a.logC < d->log_b) a.logC = d->log_b;
            a.src_stride = cs;
            const bool fuse = ntt_fast_ok(a, NTT_DIT_LDE);
            if (fuse) {
                a.src = d_coef;                                   // raw DIF output: prepared at the load
                a.prep = 1; a.prep_log_n = d->log_n; a.prep_log_b = d->log_b; a.prep_ninv_mont = d->ninv_mont;
                a.prep_nd = d->plan.nd; a.prep_wtab = d->W.view();
                for (uint32_t t = 0; t < d->plan.nd; ++t) a.prep_bits[t] = d->plan.bits[t];
            } else {
                HIPCHK(launch_coef_prepare(d_coef, d_prep, pa, s, prof, batch, cs, cs));
                a.src = d_prep;
            }
            HIPCHK(launch_ntt_pass(a, NTT_DIT_LDE, s, prof));
        } else {
            a.src = d_out;
            HIPCHK(launch_ntt_pass(a, NTT_DIT, s, prof));
        }
        inner += d->plan.bits[q];
    }
    return ZK_OK;
}

// prover.rs:101-173 pointwise on the domain.
int compose_args(const zk_dom* d, const uint32_t* d_f, uint32_t* d_cp, uint32_t first, uint32_t last,
                 const uint32_t alpha_raw[3], ComposeArgs& a) {
    a = ComposeArgs{};
    a.f = d_f; a.inv_xm1 = d->d_inv_xm1; a.cp = d_cp;
    a.logN = d->L; a.log_b = d->log_b;
    a.htab = d->H.view();
    a.w_mont = d->shift_mont; a.gm1_mont = d->gm1_mont; a.gm2_mont = d->gm2_mont; a.gm3_mont = d->gm3_mont;
    a.first = first % P; a.last = last % P;
    uint32_t a0 = alpha_raw[0] % P, a1 = alpha_raw[1] % P, a2 = alpha_raw[2] % P;   // field.rs:20-24
    a.alpha0_mont = to_mont(a0);
    a.alpha1g2_mont = to_mont(mulmod(a1, mulmod(d->g, d->g)));
    for (size_t r = 0; r < d->B; ++r) {
        if (d->inv_den[r] == 0) return fail(ZK_ERR_INVALID, "compose: x^n = 1 on the domain");
        a.zz[r] = to_mont(to_mont(mulmod(a2, d->inv_den[r])));
    }
    return ZK_OK;
}
int dom_compose(const zk_dom* d, const uint32_t* d_f, uint32_t* d_cp, uint32_t first, uint32_t last,
                const uint32_t alpha_raw[3], hipStream_t s, Profiler* prof) {
    ComposeArgs a;
    int rc = compose_args(d, d_f, d_cp, first, last, alpha_raw, a);
    if (rc) return rc;
    HIPCHK(launch_compose(a, s, prof));
    return ZK_OK;
}

// cp over E (ext.hpp): alpha_raw = alpha0.c0, alpha0.c1, alpha1.c0, alpha1.c1, alpha2.c0, alpha2.c1, the order they are drawn in;
// d_cp takes two planes of N words.  Component 0 is set up by compose_args itself, so plane 0 is dom_compose's cp for it.
int dom_compose_ext(const zk_dom* d, const uint32_t* d_f, uint32_t* d_cp, uint32_t first, uint32_t last, const uint32_t alpha_raw[6],
                    hipStream_t s, Profiler* prof) {
    const uint32_t c0[3] = {alpha_raw[0], alpha_raw[2], alpha_raw[4]}, c1[3] = {alpha_raw[1], alpha_raw[3], alpha_raw[5]};
    ComposeExtArgs e;
    ComposeArgs one;
    int rc = compose_args(d, d_f, d_cp, first, last, c0, e.a);
    if (!rc) rc = compose_args(d, d_f, d_cp, first, last, c1, one);
    if (rc) return rc;
    e.alpha0_mont1 = one.alpha0_mont; e.alpha1g2_mont1 = one.alpha1g2_mont;
    for (size_t r = 0; r < 32; ++r) e.zz1[r] = one.zz[r];
    HIPCHK(launch_compose_ext(e, s, prof));
    return ZK_OK;
}

// polynomial.rs:385-400 + prover.rs:204-211 in evaluation form: layer of 2^log_m values at
// x_i = (shift h^i)^(2^round) -> 2^(log_m-1) values.
int fold_args(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t beta_raw, FoldArgs& a) {
    if (log_m < 1 || log_m + round != d->L) return fail(ZK_ERR_INVALID, "fold: layer size 2^%u does not match round %u of a 2^%u domain", log_m, round, d->L);
    a = FoldArgs{};
    a.in = d_in; a.out = d_out; a.log_m = log_m; a.round = round;
    a.hinv = d->Hinv.view(); a.L = d->L;
    a.inv2_mont = d->inv2_mont;
    a.c_mont = to_mont(mulmod(beta_raw % P, d->fold_k[round]));   // beta * w^(-2^r) / 2
    return ZK_OK;
}
int dom_fold(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t beta_raw,
             hipStream_t s, Profiler* prof) {
    FoldArgs a;
    int rc = fold_args(d, d_in, d_out, log_m, round, beta_raw, a);
    if (rc) return rc;
    HIPCHK(launch_fri_fold(a, s, prof));
    return ZK_OK;
}

// `steps` successive folds (rounds round .. round + steps - 1) with the challenges beta, beta^2, beta^4, ... in one pass: layer of
// 2^log_m values -> 2^(log_m - steps).  Every constant that depends on the challenge or on a root of unity, not on the position,
// is folded here into the launch arguments (FoldMultiArgs::c_mont).
int fold_multi_args(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t steps, uint32_t beta_raw,
                    FoldMultiArgs& a) {
    if (steps < 1 || steps > 3) return fail(ZK_ERR_INVALID, "fold: steps must be 1..3 (got %u)", steps);
    if (log_m < steps || log_m + round != d->L)
        return fail(ZK_ERR_INVALID, "fold: layer size 2^%u does not match round %u + %u steps of a 2^%u domain", log_m, round, steps, d->L);
    a = FoldMultiArgs{};
    a.in = d_in; a.out = d_out; a.log_m = log_m; a.round = round; a.steps = steps;
    a.hinv = d->Hinv.view();
    a.scale_mont = to_mont(invmod(1u << steps));
    const uint32_t S = 1u << steps;
    const uint32_t om_inv = invmod(powmod(d->h, (uint64_t)d->N >> steps));   // h^(N / S): index + m / S multiplies the point by it
    uint32_t bk = beta_raw % P, ok = om_inv;                                  // beta^(2^k), w_S^(-2^k)
    for (uint32_t k = 0; k < steps; ++k) {
        const uint32_t base = mulmod(bk, mulmod(d->fold_k[round + k], 2));   // beta^(2^k) * w^(-2^(r+k))
        uint32_t tw = 1;
        for (uint32_t t = 0; t < (S >> (k + 1)); ++t) { a.c_mont[S - (S >> k) + t] = to_mont(mulmod(base, tw)); tw = mulmod(tw, ok); }
        bk = mulmod(bk, bk); ok = mulmod(ok, ok);
    }
    return ZK_OK;
}
// The same for a proof-major batch (FoldMultiBatchArgs): the challenge-independent part of every constant (fold_multi_args with
// beta = 1); the challenges stay on the device, d_work takes the per-proof constants.
int fold_multi_batch_args(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t steps,
                          const uint32_t* d_beta_raw, uint32_t beta_stride, uint32_t* d_work, uint32_t batch, FoldMultiBatchArgs& a) {
    a = FoldMultiBatchArgs{};
    if (int rc = fold_multi_args(d, d_in, d_out, log_m, round, steps, 1u, a.a)) return rc;
    if (batch < 1 || ((uint64_t)batch << log_m) > ((uint64_t)1 << 32))
        return fail(ZK_ERR_INVALID, "fold: a batch of %u layers of 2^%u values does not fit 2^32 values", batch, log_m);
    a.beta_raw = d_beta_raw; a.beta_stride = beta_stride; a.cb = d_work; a.batch = batch;
    return ZK_OK;
}
int dom_fold_multi_batch(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t steps,
                         const uint32_t* d_beta_raw, uint32_t beta_stride, uint32_t* d_work, uint32_t batch, hipStream_t s, Profiler* prof) {
    FoldMultiBatchArgs a;
    int rc = fold_multi_batch_args(d, d_in, d_out, log_m, round, steps, d_beta_raw, beta_stride, d_work, batch, a);
    if (rc) return rc;
    HIPCHK(launch_fri_fold_multi_batch(a, s, prof));
    return ZK_OK;
}
int dom_fold_multi(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t steps, uint32_t beta_raw,
                   hipStream_t s, Profiler* prof) {
    if (steps == 1) return dom_fold(d, d_in, d_out, log_m, round, beta_raw, s, prof);
    FoldMultiArgs a;
    int rc = fold_multi_args(d, d_in, d_out, log_m, round, steps, beta_raw, a);
    if (rc) return rc;
    HIPCHK(launch_fri_fold_multi(a, s, prof));
    return ZK_OK;
}

// The group fold over E (ext.hpp): values and the challenge beta = (beta_raw[0], beta_raw[1]) in E, squared in E between the steps;
// d_in is two planes of 2^log_m words, d_out two planes of 2^(log_m - steps).  The root-of-unity part of every constant is
// fold_multi_args' with beta = 1; steps = 1 takes the same kernel (there is no separate one-round form over E).
int fold_multi_ext_args(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t steps,
                        const uint32_t beta_raw[2], FoldMultiExtArgs& a) {
    FoldMultiArgs b;
    if (int rc = fold_multi_args(d, d_in, d_out, log_m, round, steps, 1u, b)) return rc;
    a = FoldMultiExtArgs{};
    a.in = d_in; a.out = d_out; a.log_m = log_m; a.round = round; a.steps = steps;
    a.hinv = b.hinv; a.scale_mont = b.scale_mont;
    const uint32_t S = 1u << steps;
    Ext bk = ext_reduce(beta_raw[0], beta_raw[1]);                             // beta^(2^k)
    for (uint32_t k = 0; k < steps; ++k) {
        for (uint32_t t = 0; t < (S >> (k + 1)); ++t) {
            const uint32_t j = S - (S >> k) + t, root = mont_mul(b.c_mont[j], 1u);   // back from Montgomery form
            a.c[j] = ext_const(Ext{mulmod(bk.c0, root), mulmod(bk.c1, root)});
        }
        bk = ext_mul(bk, bk);
    }
    return ZK_OK;
}
int dom_fold_multi_ext(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t steps,
                       const uint32_t beta_raw[2], hipStream_t s, Profiler* prof) {
    FoldMultiExtArgs a;
    int rc = fold_multi_ext_args(d, d_in, d_out, log_m, round, steps, beta_raw, a);
    if (rc) return rc;
    HIPCHK(launch_fri_fold_multi_ext(a, s, prof));
    return ZK_OK;
}

// The same for a proof-major batch of layers of E (FoldMultiExtBatchArgs): the root-of-unity part of every constant here, the
// challenges and their powers in E on the device.
int dom_fold_multi_ext_batch(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t steps,
                             const uint32_t* d_beta0_raw, uint32_t stride0, const uint32_t* d_beta1_raw, uint32_t stride1, uint32_t* d_work,
                             uint32_t batch, hipStream_t s, Profiler* prof) {
    FoldMultiExtBatchArgs a{};
    if (int rc = fold_multi_args(d, d_in, d_out, log_m, round, steps, 1u, a.a)) return rc;
    if (batch < 1 || ((uint64_t)batch << log_m) > ((uint64_t)1 << 32))
        return fail(ZK_ERR_INVALID, "fold: a batch of %u layers of 2^%u values does not fit 2^32 values", batch, log_m);
    a.beta0_raw = d_beta0_raw; a.stride0 = stride0; a.beta1_raw = d_beta1_raw; a.stride1 = stride1; a.cb = d_work; a.batch = batch;
    HIPCHK(launch_fri_fold_multi_ext_batch(a, s, prof));
    return ZK_OK;
}

// FRI layer `round` (2^log_m <= 4096 values at (shift h^i)^(2^round)) -> d_out[0] = non-zero coefficients of degree >= bound,
// d_out[1 + k] = coefficient k of its interpolant in X, k < 2^log_m (FinalPolyArgs); `polys` layers / outputs in_stride / out_stride apart
int dom_final_poly(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t bound, hipStream_t s,
                   Profiler* prof, uint32_t polys, size_t in_stride, size_t out_stride) {
    if (log_m < 1 || log_m > kFinalPolyMaxLog || log_m + round != d->L)
        return fail(ZK_ERR_INVALID, "final polynomial: layer size 2^%u does not match round %u of a 2^%u domain, or exceeds 2^%u values", log_m, round, d->L, kFinalPolyMaxLog);
    FinalPolyArgs a{};
    a.in = d_in; a.out = d_out; a.in_stride = in_stride; a.out_stride = out_stride; a.polys = polys;
    a.log_m = log_m; a.bound = bound;
    a.hinv = d->Hinv.view(); a.L = d->L;
    a.minv_mont = to_mont(invmod(1u << log_m));
    a.sinv_mont = to_mont(mulmod(d->fold_k[round], 2));      // w^(-2^r)
    HIPCHK(launch_fri_final_poly(a, s, prof));
    return ZK_OK;
}

// `batch` layers `round`, proof-major ([batch][2^log_m]) -> d_out = [batch][1 + bound]: per layer its count of non-zero coefficients of
// degree >= bound, then coefficients 0 .. bound - 1 (launch_fri_final_poly_batch)
int dom_final_poly_batch(const zk_dom* d, const uint32_t* d_in, uint32_t* d_out, uint32_t log_m, uint32_t round, uint32_t bound, uint32_t batch,
                         hipStream_t s, Profiler* prof) {
    if (log_m < 1 || log_m > kFinalPolyMaxLog || log_m + round != d->L || bound < 1 || bound > (1u << log_m) || batch < 1)
        return fail(ZK_ERR_INVALID, "final polynomials: %u layers of 2^%u values, bound %u, do not match round %u of a 2^%u domain (at most 2^%u values)",
                    batch, log_m, bound, round, d->L, kFinalPolyMaxLog);
    FinalPolyArgs a{};
    a.in = d_in; a.out = d_out; a.in_stride = (size_t)1 << log_m; a.out_stride = (size_t)bound + 1; a.polys = batch;
    a.log_m = log_m; a.bound = bound;
    a.hinv = d->Hinv.view(); a.L = d->L;
    a.minv_mont = to_mont(invmod(1u << log_m));
    a.sinv_mont = to_mont(mulmod(d->fold_k[round], 2));      // w^(-2^r)
    HIPCHK(launch_fri_final_poly_batch(a, s, prof));
    return ZK_OK;
}

// Waits until the mailbox carries the sequence number of the last commit launch (polling host-coherent
// memory: no blit kernel, no stream synchronisation on the commit -> challenge path).
int wait_flag(const uint32_t* flag, uint32_t want, hipStream_t stream, int (*poll)(void*), void* poll_user, double timeout_s) {
    auto t0 = std::chrono::steady_clock::now();
    uint64_t spins = 0;
    while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != want) {
#if !defined(__HIP_DEVICE_COMPILE__) && (defined(__x86_64__) || defined(__i386__))
        __builtin_ia32_pause();                          // be kind to the sibling hardware thread
#endif
        if (poll && (++spins & 0xFFF) == 0) {
            if (int prc = poll(poll_user)) return prc;
        } else if (!poll) {
            ++spins;
        }
        if ((spins & 0xFFFF) == 0) {
            hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess && __atomic_load_n(flag, __ATOMIC_ACQUIRE) != want)
                return fail(ZK_ERR_HIP, "merkle digests were never posted (stream drained)");
            if (q != hipSuccess && q != hipErrorNotReady)
                return fail(ZK_ERR_HIP, "device error while waiting for merkle digests: %s", hipGetErrorString(q));
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
                return fail(ZK_ERR_HIP, "timed out after %.0f s waiting for merkle digests", timeout_s);
        }
    }
    return ZK_OK;
}

double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// merkle.rs:54-71: node indices of the authentication path of `leaf` in a tree of m leaves
void path_nodes(size_t m, size_t leaf, std::vector<size_t>& out) {
    size_t i = leaf + (2 * m - 1) / 2;
    while (i != 0) {
        if (i % 2 == 0) { out.push_back(i - 1); i -= 2; }
        else { out.push_back(i + 1); i -= 1; }
        i >>= 1;
    }
}

}  // namespace impl
}  // namespace zk
