// verify.hip -- batched proof verification on the device (zk_verifier_*).  The single-proof entry points (zk_verify*) are in
// zkstark.hip; the CPU verifier itself, one for every folding factor, is transcript.hpp.
//
// The result of every proof is the number the CPU verifier stops at (transcript.hpp: verify_transcript, then verify_proof, with the
// ProofFormat of the handle), for every input.  The device gets there without a per-proof parser:
//   * once the length is fixed, every field of a proof sits at a fixed offset if every u64 path count has its expected value.  The host
//     lays the format out once per run, from ProofFormat::for_each_head / for_each_tuple, into a table of at most 32 trees that travels
//     with the launch arguments (ProofLayout): the header words of the alphas, of every beta and tree commitment and of the free term, the
//     words of the f and cp tuples, and per group the first word of its opening and the digests of its paths.  The kernels read every
//     offset from it; none is restated in closed form.  The algebra kernel checks the counts; a proof whose counts differ is "malformed"
//     and the host runs verify_proof on it (only garbage takes that path).  On the fixed layout the checks -1, -3, -(200 + j) and -8
//     cannot fail;
//   * every other check runs in parallel and posts an order key (query * keys + position, the order verify_proof visits them in); the
//     smallest key per proof is the first failure (atomicMin), whichever lane finishes first;
//   * strict mode: a transcript failure wins (verify_transcript runs first on the CPU), so it has its own result.
// The raw-value rules of verify_proof are kept: values are reduced % P before arithmetic, but cp(x) is compared unreduced with cp0, and
// the FRI expectation (value 0 of the next group, or the free term) unreduced with a reduced calc.  Leaf hashes take the raw word.
//
// One format, of which every setter's default is the degenerate case:
//   * folding factor 2^K (zk_verifier_set_fold, K = 1..3): the R rounds come in G = ceil(R / K) groups, group j opens the s_j = 2^steps_j
//     values of its input layer (round r0 = jK) and only the last group can be short.  K = 1 is G = R groups of two values.  The fold
//     comparison inverts x once per (proof, query) and squares the inverse from round to round; the inverse powers of the 8th root of
//     unity that tell the s points of a group apart come with the launch arguments (residues are canonical, so an algebraically equal
//     evaluation is bit-exact);
//   * leaf format (zk_verifier_set_coset_leaves).  One-value leaves: a query is four tuples (f(x), f(gx), f(g^2 x), cp(x)) of a value, a
//     count and a path, then per group its s_j values and s_j paths.  Order keys, 5 + 9G per query: 0 (-2), 1..4 (-4..-7), 5 + j (the
//     fold comparison of group j, -(100 + j)), 5 + G + 8j + u (path u of group j: -(300 + j) for u = 0, -(400 + j) for u >= 1).  Coset
//     leaves: three f tuples, then per group its s_j slot words in slot order, ONE count and ONE path.  Value u of group j is slot
//     (rot + u) & (s - 1) with rot = (tp % len) >> (log len - steps): the kernels read it at that address, and cp(x) is value 0 of group
//     0.  Order keys, 4 + 2G per query: 0 (-2), 1..3 (-4..-6), 4 + j (-(100 + j)), 4 + G + j (the path of group j, -(300 + j)); -7 and
//     -(400 + j) cannot occur;
//   * early stop (zk_verifier_set_fri_stop, D = 0..8): the groups are those of the R' = log_n - D folded rounds, and the launch arguments
//     carry R', G' and the last group's steps as R, G and ls (the cp0 relation alone keeps log_n).  With D != 0 the header has no last
//     tree, and the 2^D coefficients stand where the free term was: the last group's fold is compared with p(x^(2^R')) by Horner over
//     the coefficients, each reduced % P on reading, canonical against canonical.  A uniform branch on D;
//   * Merkle caps (zk_verifier_set_merkle_cap, c = 0..8): every tree commitment is the tree's 2^ce digests and every path is ce digests
//     shorter, with ce = min(c, lg - 1) per tree.  A path walks lg - ce levels and is compared with cap entry leaf >> (lg - ce); the
//     transcript commits the 8 * 2^ce words of a cap in one piece.  c = 0 is one digest per cap, the root;
//   * shared proofs (zk_verifier_set_shared, lb = 0..8, with or without row leaves): ONE proof of M = 2^lb statements, M public values
//     per proof; the layout also says how many f tuples a query has (nft = 3M, or 3 rows; lb = 0: 3), how long one is, and where
//     statement p's share of the f commitment starts.
// Three kernels check a plain proof (lb = 0), one instance each per leaf format (and hash): verify_algebra_kernel, verify_paths_kernel
// and, strict, verify_transcript_kernel.  Slot and tree are uniform per blockIdx.y, so all lanes of a wave walk paths of one length.
//
// A shared proof has five kernels, two of them further instances of the bodies above:
//   * verify_shared_algebra_kernel, one lane per (proof, query): the counts of the cp tuple, the groups and the three rows, the -2 relation
//     summed over the M statements as verify_proof sums it (three inversions per lane, three multiplications by alpha per statement), the G
//     fold comparisons of verify_algebra_kernel;
//   * verify_shared_f_paths_kernel (one-value leaves), one lane per (proof, statement) and blockIdx.y = (query, k): shared batches are few
//     proofs of many statements, so the statement is on the lane.  Each lane checks the count of its own tuple before it walks L - ce_f levels;
//   * verify_shared_row_paths_kernel (row leaves), one lane per proof and blockIdx.y = (query, row): the row's leaf is host_coset_leaf_hash
//     with s = M bit for bit -- the coset leaf up to M = 8, streamed SHA-256 blocks or the field hash's chain from M = 16 on;
//   * verify_shared_paths_kernel: the cp tuple and the group paths, the slots >= 3 of verify_paths_kernel behind the nft f tuples;
//   * verify_shared_transcript_kernel (strict), one lane per proof: the f commitment in one commit, 3M alphas, nft f tuples per query.  This
//     chain is serial in the proof's length, which with one-value leaves grows with M q.
// Its order keys are query * keys + position in verify_proof's visiting order: 0 (-2), 1 + 3p + k (-(4 + k) for statement p; rows: 1 + k),
// with one-value leaves nft + 1 (-7), then the G fold comparisons, then the group paths (8 per group, or 1 with coset leaves);
// keys = nft + 2 + 9G, or nft + 1 + 2G with coset leaves: at nft = 3 the keys of a plain proof (order_key_to_check).
//
// A proof over E = F_P[u] / (u^2 - 5) (zk_verifier_set_ext, ext_log = 1; transcript.hpp "ext"; never shared) has three kernels
// of its own, so that the kernels above are what they were.  On the wire the alphas are six words, a beta two, the free term two (D != 0: two
// planes of 2^D coefficients), and every cp or group tuple sends 2 s value words where it sent s: the component-0 words, then the
// component-1 words.  The layout table gets these sizes from the same two walks (the tuple walk with the words per value); the order keys
// are a plain proof's.
//   * verify_ext_algebra_kernel, one lane per (proof, query): the counts behind the doubled value words; the -2 relation per component
//     with the base-field quotients computed once; fold_group_ext, the fold in E against base-field points; the expectation in both words
//     (D != 0: one Horner loop over both planes).  A comparison fails when either component differs;
//   * verify_ext_paths_kernel, one lane per proof, blockIdx.y = (query, slot): the f slots are one-word leaves; every other leaf is the row
//     leaf of the value's words (host_coset_leaf_hash): the 2 words of one value of E, not adjacent in a group tuple, or with coset leaves
//     the 2 s contiguous words of the group, 16 of them for a full group at K = 3 (the row leaf of M = 16: two SHA-256 blocks, or two
//     links of the field hash's chain);
//   * verify_ext_transcript_kernel (strict): replay_transcript with two draws per challenge of E and two words per value, 6 + 2G + q
//     challenges.
// No kernel uses scratch or LDS; at most 116 VGPRs.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "internal.hpp"
#include "fieldhash_f64.hpp"
#include "sha256.hpp"
#include "transcript.hpp"

using namespace zk;
using namespace zk::impl;

namespace zk {
namespace {

// The field hash's round constants for this translation unit (the build links without -fgpu-rdc, so kernels.hip's copy is
// not visible here); filled once per device by ensure_verify_consts.
__constant__ FieldHashConsts64 g_vfh_consts64;

constexpr int32_t kNoFailure = 0x7f7f7f7f;   // the memset pattern of the per-proof key: above every order key
constexpr uint32_t kVerifyThreads = 64;      // one wave per workgroup: the proofs of a batch spread over as many SIMDs as possible

// Where the fields of a proof sit, in 32-bit words (every field of the wire format is 4-byte aligned and ProofFormat::data_len is a
// multiple of 4), for the fixed layout: filled by verifier_chunk from ProofFormat.  Group j < G opens the tree over its input layer;
// entry G of capw / capn is the tree over the last layer (D = 0), which nothing opens.
constexpr uint32_t kLayoutTrees = 32;
struct ProofLayout {
    uint32_t fplen, fwords;     // an f path has L - ce_f digests; an f tuple 3 + 8 fplen words
    uint32_t cpplen, cpwords;   // one-value leaves: the cp(x) tuple, a path into the tree of group 0
    uint32_t fcapn, aw, ftw;    // words of f's cap (it starts the proof); header word of alpha0; of the free term / the coefficients
    uint32_t bw[kLayoutTrees];     // header word of group j's beta
    uint32_t capw[kLayoutTrees];   // header word of the cap of the tree over group j's input layer
    uint32_t capn[kLayoutTrees];   // its words: 8 * 2^ce
    uint32_t plen[kLayoutTrees];   // digests of a path into that tree: lg - ce
    uint32_t gw[kLayoutTrees];     // first word of group j's opening, counted from the first word of the query
    // shared proofs (ProofFormat::lb / rows; the kernels of a plain proof read none of these).  fwords is then the words of ONE f tuple,
    // 3 + 8 fplen for a statement's value or 2^lb + 2 + 8 fplen for a row, and the cp tuple (coset: group 0) follows the nft f tuples
    uint32_t nft;               // f tuples per query: 3 * 2^lb, or 3 rows (a plain proof: 3)
    uint32_t fshare;            // words of one statement's share of the f commitment: 8 * 2^ce_f (rows: unused, one cap for all)
    uint32_t lb;                // log2 of the statements of a proof
    uint32_t keys;              // order keys per query (order_key_to_check): nft + 2 + 9G, or nft + 1 + 2G with coset leaves
    uint32_t ext;               // ProofFormat::ext: 1 = cp, the groups and the free term hold values of E, two words each (the ext kernels)
};

// The launch arguments of every kernel: the buffers, the sizes and constants of the format, and the layout.
struct VerifyArgs {
    const uint32_t* proofs;     // [count][words]
    const uint32_t* pub;        // [count] public_last (raw)
    const uint32_t* states;     // [count][8] Proof.state bytes as loaded words, or null
    int32_t* best;              // [count] smallest order key of a failed check (kNoFailure: none)
    uint32_t* malformed;        // [count] 1: a path count differs from the fixed layout
    int32_t* tcode;             // [count] transcript result: 0, -(1000 + k), -1999
    uint32_t count, words, q, R, L, B, N;
    uint32_t log_n, h, gm1, gm2, gm3;
    uint32_t gw;                // words of the grinding nonce after the free term: 0 or 2 (the query raws follow it)
    uint32_t gmask;             // grinding: the state after the nonce commit must have (word 0 & gmask) == 0
    uint32_t qbase;             // first word of query 0's openings
    uint32_t per_q;             // words of one query's openings
    // folding factor 2^K: G groups of K rounds, the last one of ls <= K (K = 1: G = R groups of two values); constants in Montgomery form
    uint32_t K, G, ls;
    uint32_t inv2m, wm1, wm2, wm3;   // 1/2 and w, w^2, w^3 for w = the inverse of the primitive 8th root of unity h^(N/8)
    uint32_t D;                 // early stop: 2^D coefficients at a.t.ftw (R, G, ls are then those of the log_n - D folded rounds)
    ProofLayout t;
};

__device__ __forceinline__ uint32_t be_word(const uint32_t* p) { return __builtin_bswap32(*p); }

// canonical residues in, canonical out (both operands < P)
__device__ __forceinline__ uint32_t dmul(uint32_t a, uint32_t b) { return mont_mul(mont_mul(a, b), R2); }
__device__ __forceinline__ uint32_t dpow(uint32_t a, uint32_t e) {
    uint32_t r = 1, b = a;
#pragma unroll 1
    for (int i = 0; i < 32; ++i) {
        const uint32_t t = dmul(r, b);
        r = (e & 1u) ? t : r;
        b = dmul(b, b);
        e >>= 1;
    }
    return r;
}
__device__ __forceinline__ uint32_t dinv(uint32_t a) { return dpow(a, P - 2); }   // invmod: 0 -> 0, as on the host

__device__ __forceinline__ uint32_t query_tp(const VerifyArgs& a, const uint32_t* pr, uint32_t qk) {
    return pr[a.qbase - a.q + qk] % (a.N - 2u * a.B);                        // tp = test_raw % (N - 2B); the raws end at qbase
}

__device__ __forceinline__ uint32_t group_steps(const VerifyArgs& a, uint32_t j) { return j + 1u < a.G ? a.K : a.ls; }
// Coset leaves: the slot that holds value 0 of group j (the one at tp % len): rot = (tp % len) >> (log len - steps)
__device__ __forceinline__ uint32_t coset_rot(const VerifyArgs& a, uint32_t tp, uint32_t j) {
    const uint32_t lg = a.L - j * a.K, steps = group_steps(a, j);
    return (tp & ((1u << lg) - 1u)) >> (lg - steps);
}

// proof.rs:63-77: the composition polynomial at x from f(x), f(gx), f(g^2 x), against the raw cp(x) of the proof: the value of
// the fourth tuple, or, with coset leaves, slot rot0 of group 0's leaf, which starts where that tuple would
// fb: words of an f tuple, aw: the header word of alpha0 (ProofLayout: fwords, aw)
__device__ __forceinline__ bool cp0_matches_at(const VerifyArgs& a, const uint32_t* pr, uint32_t p, uint32_t fq, uint32_t x, uint32_t rot0, uint32_t fb, uint32_t aw) {
    const uint32_t f_x = pr[fq] % P, f_gx = pr[fq + fb] % P, f_ggx = pr[fq + 2u * fb] % P, cp_raw = pr[fq + 3u * fb + rot0];
    const uint32_t p0 = dmul(sub(f_x, 1u), dinv(sub(x, 1u)));
    const uint32_t p1 = dmul(sub(f_x, a.pub[p] % P), dinv(sub(x, a.gm2)));
    const uint32_t num = sub(sub(f_ggx, dmul(f_gx, f_gx)), dmul(f_x, f_x));
    uint32_t xn = x;
    for (uint32_t i = 0; i < a.log_n; ++i) xn = dmul(xn, xn);
    const uint32_t den = dmul(sub(xn, 1u), dinv(dmul(dmul(sub(x, a.gm3), sub(x, a.gm2)), sub(x, a.gm1))));
    const uint32_t p2 = dmul(num, dinv(den));
    const uint32_t cp0 = add(add(dmul(pr[aw] % P, p0), dmul(pr[aw + 1u] % P, p1)), dmul(pr[aw + 2u] % P, p2));
    return cp0 == cp_raw;
}

// Early stop: p(xs) for xs = x^(2^R'), the point of the stopped layer, by Horner from the highest of the 2^D coefficients; each is
// reduced % P on reading (verify_proof does the same), the result is canonical.  xs goes to Montgomery form once, so a step is one
// mont_mul (canonical * Montgomery = canonical) and one add.  Every lane of a proof reads the same <= 256 words.
__device__ __forceinline__ uint32_t final_poly_from(const VerifyArgs& a, const uint32_t* c, uint32_t xs) {
    const uint32_t xm = mont_mul(xs, R2);
    uint32_t acc = 0u;
#pragma unroll 1
    for (uint32_t k = 1u << a.D; k-- > 0u;) acc = add(mont_mul(acc, xm), c[k] % P);
    return acc;
}

// STEPS successive reference folds (proof.rs:110-113) of the 2^STEPS values of one group, in registers: round k pairs t with
// t + cnt and divides by twice the point of t, x^(2^(r0 + k)) om^(2^k t) for the 2^STEPS-th root of unity om.  ixk comes in as
// x^-(2^r0) and leaves squared STEPS times; om^-(2^k t) is w^e with e = (8 >> STEPS) (t << k) in 0..3, a constant once unrolled.
// rot (coset leaves): value t is read from slot (rot + t) & (S - 1) of the leaf at vals; the register index stays static.
template <int STEPS>
__device__ __forceinline__ uint32_t fold_group(const VerifyArgs& a, const uint32_t* vals, uint32_t beta, uint32_t& ixk, uint32_t rot = 0u) {
    constexpr int S = 1 << STEPS;
    uint32_t v[S];
#pragma unroll
    for (int t = 0; t < S; ++t) v[t] = vals[(rot + (uint32_t)t) & (uint32_t)(S - 1)] % P;
    uint32_t bk = beta;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const uint32_t m = dmul(bk, ixk);                 // beta^(2^k) / x^(2^(r0 + k))
#pragma unroll
        for (int t = 0; t < (S >> (k + 1)); ++t) {
            const int e = (8 >> STEPS) * (t << k);
            const uint32_t lo = v[t], hi = v[t + (S >> (k + 1))];
            uint32_t h = dmul(sub(lo, hi), m);
            if (e != 0) h = mont_mul(h, e == 1 ? a.wm1 : e == 2 ? a.wm2 : a.wm3);
            v[t] = mont_mul(add(add(lo, hi), h), a.inv2m);     // ((lo + hi) + beta' (lo - hi) / point) / 2
        }
        ixk = dmul(ixk, ixk);
        bk = dmul(bk, bk);
    }
    return v[0];
}

template <int HASH>
__device__ __forceinline__ Digest vleaf(uint32_t v) {
    if constexpr (HASH == 0) return sha256_leaf(v);
    else return fieldhash_leaf64(v, g_vfh_consts64);
}
template <int HASH>
__device__ __forceinline__ Digest vinner(const Digest& l, const Digest& r) {
    if constexpr (HASH == 0) return sha256_inner(l, r);
    else return fieldhash_inner64(l, r, g_vfh_consts64);
}

// The digest of a leaf of s = 1, 2, 4 or 8 slot words, bit for bit host_coset_leaf_hash (transcript.hpp) and coset_leaf_digest
// (kernels.hip), raw words >= P included: SHA-256 is one block over the s big-endian words with the padding in place, the field
// hash the compression of (slot_0 .. slot_{s-1}, 0, ..., 0, s).  s = 1 is vleaf.  s is the same for every lane of a launch row
// (a uniform branch skips the loads past s); the words are placed with selects on static register indices.
// words_vleaf: from the s words already placed in v (v[i] = 0 for i >= s), for words that do not lie side by side in the proof (ext_vleaf).
template <int HASH>
__device__ __forceinline__ Digest words_vleaf(const uint32_t (&v)[8], uint32_t s) {
    Digest d;
    if constexpr (HASH == 0) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = i < 8 ? ((uint32_t)i == s ? 0x80000000u : v[i]) : 0u;   // v[i] is 0 for i > s
        w[8] = s == 8u ? 0x80000000u : 0u;
        w[15] = 32u * s;
#pragma unroll
        for (int i = 0; i < 8; ++i) d.w[i] = SHA_IV[i];
        sha256_compress(d.w, w);
    } else {
        uint32_t in[kFhT];
#pragma unroll
        for (int i = 0; i < kFhT; ++i) in[i] = i < 8 ? v[i] : 0u;
        in[kFhT - 1] = s;
        fh64_compress(in, d.w, g_vfh_consts64);
    }
    return d;
}
template <int HASH>
__device__ __forceinline__ Digest coset_vleaf(const uint32_t* slots, uint32_t s) {
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0u;
    v[0] = slots[0];
    if (s >= 2u) v[1] = slots[1];
    if (s >= 4u) { v[2] = slots[2]; v[3] = slots[3]; }
    if (s >= 8u) {
#pragma unroll
        for (int i = 4; i < 8; ++i) v[i] = slots[i];
    }
    return words_vleaf<HASH>(v, s);
}

// SHA-256(state || data[0 .. nw)) into state (channel.rs:19-26), streamed over sha256_compress.  nw is the same for every lane,
// so the lanes of a wave stay in lockstep; data words are read little-endian and swapped to message order.
__device__ __forceinline__ void commit_words(uint32_t (&st)[8], const uint32_t* data, uint32_t nw) {
    const uint32_t M = 8u + nw;                           // message words
    const uint32_t blocks = (4u * M + 9u + 63u) / 64u;
    uint32_t hs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) hs[i] = SHA_IV[i];
    for (uint32_t b = 0; b < blocks; ++b) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t g = 16u * b + (uint32_t)i;
            uint32_t v = 0u;
            if (i < 8 && b == 0u) v = st[i & 7];
            else if (g - 8u < nw) v = be_word(data + (g - 8u));
            else if (g == M) v = 0x80000000u;
            else if (i == 15 && b + 1u == blocks) v = 32u * M;   // bit length (the high word, i == 14, is 0)
            w[i] = v;
        }
        sha256_compress(hs, w);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = hs[i];
}

// ---- plain proofs (the file header) --------------------------------------------------------------------------------------------
// (1) layout + algebra: one lane per (proof, query).  Path counts, the cp0 relation (-2) and the G fold comparisons (-(100 + j)), for every K
// (the steps of a group select the unrolled fold) and D (a.D != 0: the last comparison is against p(x^(2^R)), a canonical value).  With
// coset leaves the values come from the rotated slots, and cp(x) is value 0 of group 0.
template <bool COSET>
__global__ void __launch_bounds__(kVerifyThreads) verify_algebra_kernel(VerifyArgs a) {
    const uint64_t lane = (uint64_t)blockIdx.x * kVerifyThreads + threadIdx.x;
    if (lane >= (uint64_t)a.count * a.q) return;
    const uint32_t p = (uint32_t)(lane / a.q), qk = (uint32_t)(lane % a.q);
    const uint32_t* pr = a.proofs + (size_t)p * a.words;
    const uint32_t keys = COSET ? 4u + 2u * a.G : 5u + 9u * a.G, first = COSET ? 4u : 5u;
    const uint32_t fq = a.qbase + qk * a.per_q;
    bool ok = true;
    for (uint32_t j = 0; j < 3; ++j) {
        const uint32_t* c = pr + fq + j * a.t.fwords + 1u;
        ok = ok && c[0] == a.t.fplen && c[1] == 0u;
    }
    if constexpr (!COSET) {
        const uint32_t* c = pr + fq + 3u * a.t.fwords + 1u;
        ok = ok && c[0] == a.t.cpplen && c[1] == 0u;
    }
#pragma unroll 1
    for (uint32_t j = 0; j < a.G; ++j) {
        const uint32_t s = 1u << group_steps(a, j), len = a.t.plen[j];
        const uint32_t* c = pr + fq + a.t.gw[j] + s;
        if constexpr (COSET) ok = ok && c[0] == len && c[1] == 0u;
        else for (uint32_t u = 0; u < s; ++u) ok = ok && c[u * (2u + 8u * len)] == len && c[u * (2u + 8u * len) + 1u] == 0u;
    }
    if (!ok) { a.malformed[p] = 1u; return; }

    const uint32_t tp = query_tp(a, pr, qk);
    const uint32_t x = dmul(GEN_W, dpow(a.h, tp));
    int32_t key = kNoFailure;
    if (!cp0_matches_at(a, pr, p, fq, x, COSET ? coset_rot(a, tp, 0u) : 0u, a.t.fwords, a.t.aw)) key = (int32_t)(qk * keys);
    uint32_t ixk = dinv(x);                               // x = 5 h^tp is never zero: the one inversion of this lane's folds
#pragma unroll 1
    for (uint32_t j = 0; j < a.G && key == kNoFailure; ++j) {
        const uint32_t* vals = pr + fq + a.t.gw[j];
        const uint32_t beta = pr[a.t.bw[j]] % P, rot = COSET ? coset_rot(a, tp, j) : 0u, steps = group_steps(a, j);
        uint32_t calc;
        if (steps == 3u) calc = fold_group<3>(a, vals, beta, ixk, rot);
        else if (steps == 2u) calc = fold_group<2>(a, vals, beta, ixk, rot);
        else calc = fold_group<1>(a, vals, beta, ixk, rot);
        uint32_t expect;
        if (j + 1u < a.G) expect = pr[fq + a.t.gw[j + 1u] + (COSET ? coset_rot(a, tp, j + 1u) : 0u)];
        else if (a.D) {
            uint32_t xs = x;
#pragma unroll 1
            for (uint32_t i = 0; i < a.R; ++i) xs = dmul(xs, xs);
            expect = final_poly_from(a, pr + a.t.ftw, xs);
        } else expect = pr[a.t.ftw];
        if (calc != expect) key = (int32_t)(qk * keys + first + j);
    }
    if (key != kNoFailure) atomicMin(&a.best[p], key);
}

// (2) paths: one lane per (proof, query, path slot).  blockIdx.y = query * slots + slot and the proof on the lane, so every lane of a wave
// walks a path of the same length from a leaf of the same width; left / right is a select per level (merkle.rs:82-110).  One-value leaves:
// 4 + sum s_j slots, f(x), f(gx), f(g^2 x), cp(x), then slot 4 + (j << K) + u = path u of group j.  Coset leaves: 3 + G slots, the three
// f values, then slot 3 + j = the leaf of group j from its s_j slot words in slot order (not rotated).  A path climbs plen = lg - ce levels
// from the leaf's position inside the sub-tree of its cap entry and is compared with entry idx >> plen of the tree's cap (ce = 0: the root).
// SHARED (a shared proof, below): the f tuples have kernels of their own, so the slots start at 3 (blockIdx.y counts from there), the
// cp tuple and the groups follow the nft f tuples, and the order keys are the shared ones (order_key_to_check).
template <int HASH, bool COSET, bool SHARED>
__device__ __forceinline__ void verify_paths(const VerifyArgs& a) {
    const uint32_t p = blockIdx.x * kVerifyThreads + threadIdx.x;
    if (p >= a.count) return;
    const uint32_t slots = (COSET ? 3u + a.G : 4u + ((a.G - 1u) << a.K) + (1u << a.ls)) - (SHARED ? 3u : 0u);
    const uint32_t qk = blockIdx.y / slots, slot = blockIdx.y % slots + (SHARED ? 3u : 0u);
    const uint32_t nft = SHARED ? a.t.nft : 3u;
    // where the keys of the fold comparisons start: after -2, the f tuples and (one-value leaves) cp(x)
    const uint32_t first = SHARED ? nft + (COSET ? 1u : 2u) : COSET ? 4u : 5u;
    const uint32_t* pr = a.proofs + (size_t)p * a.words;
    const uint32_t tp = query_tp(a, pr, qk);
    const uint32_t fq = a.qbase + qk * a.per_q;
    uint32_t val_w, path_w, plen, idx, capw, pos, s = 1u;
    if (slot < 3u) {                                      // f(x), f(gx), f(g^2 x) against f's cap
        val_w = fq + slot * a.t.fwords;
        path_w = val_w + 3u;
        plen = a.t.fplen;
        idx = tp + slot * a.B;
        capw = 0u;
        pos = 1u + slot;
    } else if (!COSET && slot == 3u) {                    // cp(x) against the cap of group 0's tree
        val_w = fq + nft * a.t.fwords;
        path_w = val_w + 3u;
        plen = a.t.cpplen;
        idx = tp;
        capw = a.t.capw[0];
        pos = first - 1u;
    } else if constexpr (COSET) {                         // the leaf of group j from its s_j slot words
        const uint32_t j = slot - 3u, steps = group_steps(a, j);
        s = 1u << steps;
        val_w = fq + a.t.gw[j];
        path_w = val_w + s + 2u;
        plen = a.t.plen[j];
        idx = tp & ((1u << (a.L - j * a.K - steps)) - 1u);
        capw = a.t.capw[j];
        pos = first + a.G + j;
    } else {                                              // value u of group j at (tp % size + u size / s) % size
        const uint32_t j = (slot - 4u) >> a.K, u = (slot - 4u) & ((1u << a.K) - 1u);
        const uint32_t gs = 1u << group_steps(a, j), gw = fq + a.t.gw[j], size = a.N >> (j * a.K);
        plen = a.t.plen[j];
        val_w = gw + u;
        path_w = gw + gs + u * (2u + 8u * plen) + 2u;
        idx = (tp % size + u * (size / gs)) % size;
        capw = a.t.capw[j];
        pos = first + a.G + 8u * j + u;
    }
    Digest cur;
    if constexpr (COSET) cur = coset_vleaf<HASH>(pr + val_w, s);
    else cur = vleaf<HASH>(pr[val_w]);
    uint32_t node = (idx & ((1u << plen) - 1u)) + (1u << plen) - 1u;   // heap index inside the sub-tree of the cap entry
    for (uint32_t lvl = 0; lvl < plen; ++lvl) {
        Digest sib;
        const uint32_t* sp = pr + path_w + 8u * lvl;
#pragma unroll
        for (int i = 0; i < 8; ++i) sib.w[i] = be_word(sp + i);
        const bool right = (node & 1u) == 0u;             // an even heap index is a right child
        Digest l, r;
#pragma unroll
        for (int i = 0; i < 8; ++i) { l.w[i] = right ? sib.w[i] : cur.w[i]; r.w[i] = right ? cur.w[i] : sib.w[i]; }
        cur = vinner<HASH>(l, r);
        node = (node - (right ? 2u : 1u)) >> 1;
    }
    const uint32_t* entry = pr + capw + 8u * (idx >> plen);   // idx < 2^lg, so the entry is one of the cap's 2^ce
    bool same = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) same = same && cur.w[i] == be_word(entry + i);
    if (!same) atomicMin(&a.best[p], (int32_t)(qk * (first + (COSET ? 2u : 9u) * a.G) + pos));
}
template <int HASH, bool COSET>
__global__ void __launch_bounds__(kVerifyThreads) verify_paths_kernel(VerifyArgs a) { verify_paths<HASH, COSET, false>(a); }

// (3) transcript (strict only): one lane per proof, the commits of verify_transcript in its order.  The order is a schedule of steps the
// same for every lane (a challenge, or a commit of nw words), walked by one loop with one commit site: the compression is inlined once and
// the state stays in registers.  A tree's commit is the 8 * 2^ce words of its cap, a tuple's its values, counts and paths' digests; D != 0
// drops the last tree and commits the 2^D coefficients where the free term was.
// SHARED (a shared proof, below): na = 3 * 2^lb alphas after the f commitment, and nft f tuples (rows: 3) in front of a query's cp tuple.
// EXT (a plain proof over E, below): a challenge of E is vw = 2 draws in a row, so 6 alphas and cb = 2 challenge steps per beta, and every
// value of cp, of a group and of the free term or the coefficients is vw words.  EXT = 0: vw = cb = 1, the schedule as it was.
template <bool COSET, bool SHARED, int EXT = 0>
__device__ __forceinline__ void replay_transcript(const VerifyArgs& a) {
    constexpr uint32_t vw = 1u << EXT, cb = vw;
    const uint32_t na = SHARED ? 3u << a.t.lb : 3u * vw, nft = SHARED ? a.t.nft : 3u;
    const uint32_t NF = nft + (COSET ? 0u : 1u);          // f tuples per query, cp(x) included
    const uint32_t p = blockIdx.x * kVerifyThreads + threadIdx.x;
    if (p >= a.count) return;
    const uint32_t* pr = a.proofs + (size_t)p * a.words;
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = 0u;
    const uint32_t R = a.G, q = a.q;
    // steps: f cap | na alphas | cap 0 | R x (cb betas, cap j + 1) | free term | [nonce] | q query raws | q x (NF f tuples, R groups)
    // D != 0: the last beta has no cap after it, and the step of the free term commits the 2^D coefficients
    const uint32_t gs = a.gw ? 1u : 0u;
    const uint32_t ft = na + (a.D ? 1u : 2u) + (cb + 1u) * R;
    const uint32_t head = ft + 1u + gs + q;
    const uint32_t steps = head + q * (NF + R);
    uint32_t cur = 0, k = 0;
    int32_t code = 0;
    for (uint32_t s = 0; s < steps; ++s) {
        bool chal = false;
        uint32_t nw;
        if (s < head) {
            chal = (s >= 1u && s <= na) || (s >= na + 2u && s < ft && (s - na - 2u) % (cb + 1u) < cb) || s >= ft + 1u + gs;
            if (chal) nw = 1u;
            else if (s == 0u) nw = a.t.fcapn;
            else if (s < ft) nw = a.t.capn[(s - na - 1u) / (cb + 1u)];   // s = na + 1: the tree of group 0; s = na + (cb + 1)(j + 1) + 1: of group j + 1 (the last layer's: entry G)
            else nw = s == ft ? vw << a.D : 2u;           // D = 0: the free term, one value
        } else {
            const uint32_t u = (s - head) % (NF + R);
            if (u < nft) nw = a.t.fwords;
            else if (!COSET && u == nft) nw = a.t.cpwords;
            else {
                const uint32_t j = u - NF, gsteps = group_steps(a, j);
                nw = COSET ? (vw << gsteps) + 2u + 8u * a.t.plen[j] : (vw + 2u + 8u * a.t.plen[j]) << gsteps;
            }
        }
        if (chal) {                                       // state word 0 (big-endian bytes 0..3) against the little-endian u32 here
            ++k;
            if (st[0] != pr[cur]) { code = -(int32_t)(1000u + k); break; }
        }
        commit_words(st, pr + cur, nw);
        cur += nw;
        if (gs && s == ft + 1u && (st[0] & a.gmask) != 0u) { code = -1998; break; }   // SHA-256(S || le64(w)) is the new state
    }
    if (code == 0) {
        bool same = true;
#pragma unroll
        for (int i = 0; i < 8; ++i) same = same && st[i] == be_word(a.states + (size_t)p * 8u + i);
        if (!same) code = -1999;
    }
    a.tcode[p] = code;
}
template <bool COSET>
__global__ void __launch_bounds__(kVerifyThreads) verify_transcript_kernel(VerifyArgs a) { replay_transcript<COSET, false>(a); }

// ---- shared proofs (the file header) ---------------------------------------------------------------------------------------------
// The order keys of a shared proof, per query (verify_proof's visiting order): 0 (-2), 1 + 3p + k (the path of statement p's f(g^k x),
// -(4 + k); rows: 1 + k, the path of row k), then with one-value leaves nft + 1 (-7), then the G fold comparisons and the group paths
// (one-value leaves: 9G keys; coset leaves: 2G keys).
__device__ __forceinline__ uint32_t shared_first(const VerifyArgs& a, bool coset) { return a.t.nft + (coset ? 1u : 2u); }   // the key of group 0's fold
__device__ __forceinline__ uint32_t shared_keys(const VerifyArgs& a, bool coset) { return shared_first(a, coset) + (coset ? 2u : 9u) * a.G; }

// (1) of a shared proof: one lane per (proof, query).  The path counts of the cp tuple and the groups, and with rows those of the three
// rows (the plain f tuples check their own: verify_shared_f_paths_kernel); the -2 relation summed over the 2^lb statements; the G fold
// comparisons of verify_algebra_kernel.  The denominators of -2 depend on x alone: the sums of alpha_i times numerator_i over the
// statements are kept Montgomery-scaled (one mont_mul per term) and meet the three inverses, scaled the other way, once at the end.  All
// residues are canonical, so the sum equals verify_proof's bit for bit.
template <bool COSET, bool ROWS>
__global__ void __launch_bounds__(kVerifyThreads) verify_shared_algebra_kernel(VerifyArgs a) {
    const uint64_t lane = (uint64_t)blockIdx.x * kVerifyThreads + threadIdx.x;
    if (lane >= (uint64_t)a.count * a.q) return;
    const uint32_t p = (uint32_t)(lane / a.q), qk = (uint32_t)(lane % a.q);
    const uint32_t* pr = a.proofs + (size_t)p * a.words;
    const uint32_t M = 1u << a.t.lb;
    const uint32_t keys = shared_keys(a, COSET), first = shared_first(a, COSET);
    const uint32_t fq = a.qbase + qk * a.per_q, cpw = fq + a.t.nft * a.t.fwords;   // cpw: the cp tuple, or group 0's leaf
    bool ok = true;
    if constexpr (ROWS) {
        for (uint32_t k = 0; k < 3; ++k) {
            const uint32_t* c = pr + fq + k * a.t.fwords + M;
            ok = ok && c[0] == a.t.fplen && c[1] == 0u;
        }
    }
    if constexpr (!COSET) ok = ok && pr[cpw + 1u] == a.t.cpplen && pr[cpw + 2u] == 0u;
#pragma unroll 1
    for (uint32_t j = 0; j < a.G; ++j) {
        const uint32_t s = 1u << group_steps(a, j), len = a.t.plen[j];
        const uint32_t* c = pr + fq + a.t.gw[j] + s;
        if constexpr (COSET) ok = ok && c[0] == len && c[1] == 0u;
        else for (uint32_t u = 0; u < s; ++u) ok = ok && c[u * (2u + 8u * len)] == len && c[u * (2u + 8u * len) + 1u] == 0u;
    }
    if (!ok) { a.malformed[p] = 1u; return; }

    const uint32_t tp = query_tp(a, pr, qk);
    const uint32_t x = dmul(GEN_W, dpow(a.h, tp));
    int32_t key = kNoFailure;
    {   // proof.rs:63-77 summed over the statements, as verify_proof sums it
        uint32_t xn = x;
        for (uint32_t i = 0; i < a.log_n; ++i) xn = dmul(xn, xn);
        const uint32_t den = dmul(sub(xn, 1u), dinv(dmul(dmul(sub(x, a.gm3), sub(x, a.gm2)), sub(x, a.gm1))));
        // inverse * R^2: a sum of mont_mul(alpha, numerator) terms (each product / R) times this, by mont_mul, is the canonical product
        const uint32_t i0 = mont_mul(mont_mul(dinv(sub(x, 1u)), R2), R2), i1 = mont_mul(mont_mul(dinv(sub(x, a.gm2)), R2), R2);
        const uint32_t i2 = mont_mul(mont_mul(dinv(den), R2), R2);
        const uint32_t* pub = a.pub + (size_t)p * M;
        const uint32_t fstep = ROWS ? 1u : 3u * a.t.fwords, kstep = a.t.fwords;   // from statement to statement, from f(g^k x) to f(g^(k+1) x)
        uint32_t s0 = 0u, s1 = 0u, s2 = 0u;
#pragma unroll 2
        for (uint32_t s = 0; s < M; ++s) {
            const uint32_t* fv = pr + fq + s * fstep;
            const uint32_t* al = pr + a.t.aw + 3u * s;
            const uint32_t f_x = fv[0] % P, f_gx = fv[kstep] % P, f_ggx = fv[2u * kstep] % P;
            const uint32_t num = sub(sub(f_ggx, dmul(f_gx, f_gx)), dmul(f_x, f_x));
            s0 = add(s0, mont_mul(al[0] % P, sub(f_x, 1u)));
            s1 = add(s1, mont_mul(al[1] % P, sub(f_x, pub[s] % P)));
            s2 = add(s2, mont_mul(al[2] % P, num));
        }
        const uint32_t cp0 = add(add(mont_mul(s0, i0), mont_mul(s1, i1)), mont_mul(s2, i2));
        if (cp0 != pr[cpw + (COSET ? coset_rot(a, tp, 0u) : 0u)]) key = (int32_t)(qk * keys);
    }
    uint32_t ixk = dinv(x);                               // x = 5 h^tp is never zero: the one inversion of this lane's folds
#pragma unroll 1
    for (uint32_t j = 0; j < a.G && key == kNoFailure; ++j) {
        const uint32_t* vals = pr + fq + a.t.gw[j];
        const uint32_t beta = pr[a.t.bw[j]] % P, rot = COSET ? coset_rot(a, tp, j) : 0u, steps = group_steps(a, j);
        uint32_t calc;
        if (steps == 3u) calc = fold_group<3>(a, vals, beta, ixk, rot);
        else if (steps == 2u) calc = fold_group<2>(a, vals, beta, ixk, rot);
        else calc = fold_group<1>(a, vals, beta, ixk, rot);
        uint32_t expect;
        if (j + 1u < a.G) expect = pr[fq + a.t.gw[j + 1u] + (COSET ? coset_rot(a, tp, j + 1u) : 0u)];
        else if (a.D) {
            uint32_t xs = x;
#pragma unroll 1
            for (uint32_t i = 0; i < a.R; ++i) xs = dmul(xs, xs);
            expect = final_poly_from(a, pr + a.t.ftw, xs);
        } else expect = pr[a.t.ftw];
        if (calc != expect) key = (int32_t)(qk * keys + first + j);
    }
    if (key != kNoFailure) atomicMin(&a.best[p], key);
}

// One path of one-value or coset / row leaves from digest `cur` of leaf idx: plen levels up inside the sub-tree of its cap entry, then
// the comparison with entry idx >> plen of the cap at `cap` (the walk of verify_paths).
template <int HASH>
__device__ __forceinline__ bool path_misses(Digest cur, const uint32_t* path, uint32_t plen, uint32_t idx, const uint32_t* cap) {
    uint32_t node = (idx & ((1u << plen) - 1u)) + (1u << plen) - 1u;   // heap index inside the sub-tree of the cap entry
    for (uint32_t lvl = 0; lvl < plen; ++lvl) {
        Digest sib;
        const uint32_t* sp = path + 8u * lvl;
#pragma unroll
        for (int i = 0; i < 8; ++i) sib.w[i] = be_word(sp + i);
        const bool right = (node & 1u) == 0u;             // an even heap index is a right child
        Digest l, r;
#pragma unroll
        for (int i = 0; i < 8; ++i) { l.w[i] = right ? sib.w[i] : cur.w[i]; r.w[i] = right ? cur.w[i] : sib.w[i]; }
        cur = vinner<HASH>(l, r);
        node = (node - (right ? 2u : 1u)) >> 1;
    }
    const uint32_t* entry = cap + 8u * (idx >> plen);
    bool same = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) same = same && cur.w[i] == be_word(entry + i);
    return !same;
}

// (2a) the f paths of a shared proof with one-value leaves: one lane per (proof, statement), blockIdx.y = query * 3 + k.  A shared batch
// is few proofs of many statements, so the statement is on the lane: one proof of 64 statements fills a wave, and every lane walks
// L - ce_f levels.  Tuple 3p + k of the query holds f_p(g^k x); its path lands in statement p's share of the f commitment.  Each lane
// checks the u64 count of its own tuple (the algebra kernel does not) before it walks.
template <int HASH>
__global__ void __launch_bounds__(kVerifyThreads) verify_shared_f_paths_kernel(VerifyArgs a) {
    const uint64_t lane = (uint64_t)blockIdx.x * kVerifyThreads + threadIdx.x;
    if (lane >= ((uint64_t)a.count << a.t.lb)) return;
    const uint32_t p = (uint32_t)(lane >> a.t.lb), st = (uint32_t)lane & ((1u << a.t.lb) - 1u);
    const uint32_t qk = blockIdx.y / 3u, k = blockIdx.y % 3u;
    const uint32_t* pr = a.proofs + (size_t)p * a.words;
    const uint32_t* tup = pr + a.qbase + qk * a.per_q + (3u * st + k) * a.t.fwords;
    if (tup[1] != a.t.fplen || tup[2] != 0u) { a.malformed[p] = 1u; return; }
    const uint32_t idx = query_tp(a, pr, qk) + k * a.B;
    if (path_misses<HASH>(vleaf<HASH>(tup[0]), tup + 3u, a.t.fplen, idx, pr + st * a.t.fshare))
        atomicMin(&a.best[p], (int32_t)(qk * a.t.keys + 1u + 3u * st + k));
}

// The digest of a row of M = 2^lb values, bit for bit host_coset_leaf_hash (transcript.hpp), raw words >= P included.  M <= 8: the coset
// leaf.  M >= 16, SHA-256: M / 16 data blocks (a value is its big-endian message word), then the padding block; field hash: the chain of
// fieldhash_row_leaf, M / 8 compressions with word 15 = M in the first (row_path_misses).  The block loop is not unrolled; the next
// SHA-256 block is loaded before the current one is compressed, and only the chaining state lives across blocks (row_leaf_hash_kernel,
// with the values contiguous here).  M is the same for every lane of a launch.
template <int HASH>
__device__ __forceinline__ Digest row_vleaf(const uint32_t* vals, uint32_t M) {
    static_assert(HASH == 0, "the field hash's row leaf is part of its path walk: row_path_misses");
    if (M <= 8u) return coset_vleaf<HASH>(vals, M);
    Digest d;
    {
        const uint32_t nb = M / 16u;
        uint32_t cur[16], nx[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { cur[u] = vals[u]; nx[u] = 0u; }
#pragma unroll
        for (int i = 0; i < 8; ++i) d.w[i] = SHA_IV[i];
#pragma unroll 1
        for (uint32_t k = 0; k < nb; ++k) {
            if (k + 1u < nb) {
                const uint32_t* src = vals + 16u * (k + 1u);
#pragma unroll
                for (int u = 0; u < 16; ++u) nx[u] = src[u];
            }
            sha256_compress(d.w, cur);
#pragma unroll
            for (int u = 0; u < 16; ++u) cur[u] = nx[u];
        }
        uint32_t pad[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 32u * M};
        sha256_compress(d.w, pad);
    }
    return d;
}

// The path of a row: its leaf, plen levels up, the comparison with cap entry idx >> plen.  The field hash's leaf is one loop of
// max(M / 8, 1) compressions whose first trip is the first chunk (v_0 .. v_7, or with M < 8 the M values and zeros; then 0, .., 0, M), so
// the kernel holds two inlined compressions, the leaf's and the inner node's, as the paths kernels of one-value leaves do.
// pr: the proof; roww: the first word of the row tuple (M values, the count, plen digests), the same for every lane; the cap is at word 0.
// fh_row_chain: the chain from its first chunk `in` (v_0 .. v_7, 0, .., 0, M) on; vals: the row's first word, read from word 8 on.
__device__ __forceinline__ Digest fh_row_chain(uint32_t (&in)[kFhT], const uint32_t* vals, uint32_t M) {
    const uint32_t nb = M > 8u ? M / 8u : 1u;
    Digest cur;
    uint32_t k = 1u;
#pragma unroll 1
    for (;;) {
        fh64_compress(in, cur.w, g_vfh_consts64);
        if (k >= nb) break;
        const uint32_t* src = vals + 8u * k;
#pragma unroll
        for (int i = 0; i < 8; ++i) { in[i] = cur.w[i]; in[8 + i] = src[i]; }
        ++k;
    }
    return cur;
}
template <int HASH>
__device__ __forceinline__ bool row_path_misses(const uint32_t* pr, uint32_t roww, uint32_t M, uint32_t plen, uint32_t idx) {
    if constexpr (HASH == 0) return path_misses<0>(row_vleaf<0>(pr + roww, M), pr + roww + M + 2u, plen, idx, pr);
    else {
        uint32_t in[kFhT];
#pragma unroll
        for (int i = 0; i < 8; ++i) {                     // M < 8: the words past the values are the count and the path, loaded but not used
            const uint32_t w = pr[roww + (uint32_t)i];
            in[i] = (uint32_t)i < M ? w : 0u;
            in[8 + i] = i == 7 ? M : 0u;
        }
        return path_misses<1>(fh_row_chain(in, pr + roww, M), pr + roww + M + 2u, plen, idx, pr);
    }
}

// (2b) the f paths of a shared proof with row leaves: one lane per proof, blockIdx.y = query * 3 + k.  Row k of the query -- M values, a
// count (the algebra kernel checks it), L - ce_f digests -- is ONE leaf at index tp + k B of the one tree over the rows.
// The second launch bound asks for five waves per SIMD, the occupancy of the other field-hash paths kernels (88 VGPRs): without it the
// sixteen S-boxes of the leaf chain's full rounds are interleaved up to 130 VGPRs.
template <int HASH>
__global__ void __launch_bounds__(kVerifyThreads, 5) verify_shared_row_paths_kernel(VerifyArgs a) {
    const uint32_t p = blockIdx.x * kVerifyThreads + threadIdx.x;
    if (p >= a.count) return;
    const uint32_t qk = blockIdx.y / 3u, k = blockIdx.y % 3u, M = 1u << a.t.lb;
    const uint32_t* pr = a.proofs + (size_t)p * a.words;
    const uint32_t idx = query_tp(a, pr, qk) + k * a.B;
    if (row_path_misses<HASH>(pr, a.qbase + qk * a.per_q + k * a.t.fwords, M, a.t.fplen, idx))
        atomicMin(&a.best[p], (int32_t)(qk * a.t.keys + 1u + k));
}

// (2c) the cp tuple and the group paths of a shared proof: the slots >= 3 of verify_paths_kernel, behind the nft f tuples.
template <int HASH, bool COSET>
__global__ void __launch_bounds__(kVerifyThreads) verify_shared_paths_kernel(VerifyArgs a) { verify_paths<HASH, COSET, true>(a); }

// (3) of a shared proof (strict only): one lane per proof; the f commitment is one commit of all its words, 3 * 2^lb alphas follow it,
// and a query commits its nft f tuples one by one.  The chain is serial in the proof's length: with one-value leaves that is 3 * 2^lb
// tuples per query.
template <bool COSET>
__global__ void __launch_bounds__(kVerifyThreads) verify_shared_transcript_kernel(VerifyArgs a) { replay_transcript<COSET, true>(a); }

// ---- proofs over E = F_P[u] / (u^2 - 5) (zk_verifier_set_ext; the file header) -------------------------------------------------------
// 5 a by additions (u^2 = 5): linear, so it holds for canonical and for Montgomery residues alike
__device__ __forceinline__ uint32_t times5(uint32_t a) {
    const uint32_t a2 = add(a, a);
    return add(add(a2, a2), a);
}

// fold_group for a group of values of E: component 0 of value t is word (rot + t) & (S - 1) of the group, component 1 word S + that.  The
// points are base-field, so the multiplier of round k, beta^(2^k) / x^(2^(r0 + k)), is a base scalar times a value of E; it becomes an
// ExtConst once per round (two multiplications and 5 c1) and meets every (lo - hi) in ext.hpp's schoolbook product.  The powers of the 8th
// root and 1/2 scale both components; beta is squared in E.  Canonical residues throughout: bit-exact against verify_proof_ext.
template <int STEPS>
__device__ __forceinline__ Ext fold_group_ext(const VerifyArgs& a, const uint32_t* vals, Ext beta, uint32_t& ixk, uint32_t rot = 0u) {
    constexpr int S = 1 << STEPS;
    Ext v[S];
#pragma unroll
    for (int t = 0; t < S; ++t) {
        const uint32_t u = (rot + (uint32_t)t) & (uint32_t)(S - 1);
        v[t] = Ext{vals[u] % P, vals[(uint32_t)S + u] % P};
    }
    Ext bk = beta;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const uint32_t ixm = mont_mul(ixk, R2);
        ExtConst m;
        m.c0 = dmul(bk.c0, ixm);
        m.c1 = dmul(bk.c1, ixm);
        m.c1w = times5(m.c1);
#pragma unroll
        for (int t = 0; t < (S >> (k + 1)); ++t) {
            const int e = (8 >> STEPS) * (t << k);
            const Ext lo = v[t], hi = v[t + (S >> (k + 1))];
            Ext h = ext_mul_const(ext_sub(lo, hi), m);
            if (e != 0) h = ext_scale(h, e == 1 ? a.wm1 : e == 2 ? a.wm2 : a.wm3);
            v[t] = ext_scale(ext_add(ext_add(lo, hi), h), a.inv2m);
        }
        ixk = dmul(ixk, ixk);
        bk = Ext{add(dmul(bk.c0, bk.c0), times5(dmul(bk.c1, bk.c1))), dmul(add(bk.c0, bk.c0), bk.c1)};
    }
    return v[0];
}

// (1) of a proof over E: one lane per (proof, query).  The three f tuples are a plain proof's; the cp tuple has two value words in front of
// its count and a group 2 s_j.  p0, p1, p2 of the -2 relation are base-field and computed once; component c of cp takes alpha_i.c at word
// aw + 2 i + c and is compared raw with word c of the cp value (coset leaves: slots rot0 and s_0 + rot0 of group 0's leaf).  The fold is
// compared with both words of value 0 of the next group, with both words of the free term (raw), or with the two planes of coefficients
// (component 0 at ftw + k, component 1 at ftw + 2^D + k) by one Horner loop at the base-field point x^(2^R').  Either component posts the key.
template <bool COSET>
__global__ void __launch_bounds__(kVerifyThreads) verify_ext_algebra_kernel(VerifyArgs a) {
    const uint64_t lane = (uint64_t)blockIdx.x * kVerifyThreads + threadIdx.x;
    if (lane >= (uint64_t)a.count * a.q) return;
    const uint32_t p = (uint32_t)(lane / a.q), qk = (uint32_t)(lane % a.q);
    const uint32_t* pr = a.proofs + (size_t)p * a.words;
    const uint32_t keys = COSET ? 4u + 2u * a.G : 5u + 9u * a.G, first = COSET ? 4u : 5u;
    const uint32_t fq = a.qbase + qk * a.per_q, cpw = fq + 3u * a.t.fwords;   // cpw: the cp tuple, or group 0's leaf
    bool ok = true;
    for (uint32_t j = 0; j < 3; ++j) {
        const uint32_t* c = pr + fq + j * a.t.fwords + 1u;
        ok = ok && c[0] == a.t.fplen && c[1] == 0u;
    }
    if constexpr (!COSET) ok = ok && pr[cpw + 2u] == a.t.cpplen && pr[cpw + 3u] == 0u;
#pragma unroll 1
    for (uint32_t j = 0; j < a.G; ++j) {
        const uint32_t s = 1u << group_steps(a, j), len = a.t.plen[j];
        const uint32_t* c = pr + fq + a.t.gw[j] + 2u * s;
        if constexpr (COSET) ok = ok && c[0] == len && c[1] == 0u;
        else for (uint32_t u = 0; u < s; ++u) ok = ok && c[u * (2u + 8u * len)] == len && c[u * (2u + 8u * len) + 1u] == 0u;
    }
    if (!ok) { a.malformed[p] = 1u; return; }

    const uint32_t tp = query_tp(a, pr, qk);
    const uint32_t x = dmul(GEN_W, dpow(a.h, tp));
    int32_t key = kNoFailure;
    {   // proof.rs:63-77 with the alphas in E
        const uint32_t f_x = pr[fq] % P, f_gx = pr[fq + a.t.fwords] % P, f_ggx = pr[fq + 2u * a.t.fwords] % P;
        const uint32_t p0 = dmul(sub(f_x, 1u), dinv(sub(x, 1u)));
        const uint32_t p1 = dmul(sub(f_x, a.pub[p] % P), dinv(sub(x, a.gm2)));
        const uint32_t num = sub(sub(f_ggx, dmul(f_gx, f_gx)), dmul(f_x, f_x));
        uint32_t xn = x;
        for (uint32_t i = 0; i < a.log_n; ++i) xn = dmul(xn, xn);
        const uint32_t den = dmul(sub(xn, 1u), dinv(dmul(dmul(sub(x, a.gm3), sub(x, a.gm2)), sub(x, a.gm1))));
        const uint32_t p2 = dmul(num, dinv(den));
        const uint32_t* al = pr + a.t.aw;
        const uint32_t c0w = cpw + (COSET ? coset_rot(a, tp, 0u) : 0u), c1w = c0w + (COSET ? 1u << group_steps(a, 0u) : 1u);
        const uint32_t cp_c0 = add(add(dmul(al[0] % P, p0), dmul(al[2] % P, p1)), dmul(al[4] % P, p2));
        const uint32_t cp_c1 = add(add(dmul(al[1] % P, p0), dmul(al[3] % P, p1)), dmul(al[5] % P, p2));
        if (cp_c0 != pr[c0w] || cp_c1 != pr[c1w]) key = (int32_t)(qk * keys);
    }
    uint32_t ixk = dinv(x);                               // x = 5 h^tp is never zero: the one inversion of this lane's folds
#pragma unroll 1
    for (uint32_t j = 0; j < a.G && key == kNoFailure; ++j) {
        const uint32_t* vals = pr + fq + a.t.gw[j];
        const Ext beta{pr[a.t.bw[j]] % P, pr[a.t.bw[j] + 1u] % P};
        const uint32_t rot = COSET ? coset_rot(a, tp, j) : 0u, steps = group_steps(a, j);
        Ext calc;
        if (steps == 3u) calc = fold_group_ext<3>(a, vals, beta, ixk, rot);
        else if (steps == 2u) calc = fold_group_ext<2>(a, vals, beta, ixk, rot);
        else calc = fold_group_ext<1>(a, vals, beta, ixk, rot);
        Ext expect;
        if (j + 1u < a.G) {
            const uint32_t nw = fq + a.t.gw[j + 1u] + (COSET ? coset_rot(a, tp, j + 1u) : 0u);
            expect = Ext{pr[nw], pr[nw + (1u << group_steps(a, j + 1u))]};
        } else if (a.D) {
            uint32_t xs = x;
#pragma unroll 1
            for (uint32_t i = 0; i < a.R; ++i) xs = dmul(xs, xs);
            const uint32_t xm = mont_mul(xs, R2), nc = 1u << a.D;
            const uint32_t* c = pr + a.t.ftw;
            expect = Ext{0u, 0u};
#pragma unroll 1
            for (uint32_t k = nc; k-- > 0u;) expect = Ext{add(mont_mul(expect.c0, xm), c[k] % P), add(mont_mul(expect.c1, xm), c[nc + k] % P)};
        } else expect = Ext{pr[a.t.ftw], pr[a.t.ftw + 1u]};
        if (calc.c0 != expect.c0 || calc.c1 != expect.c1) key = (int32_t)(qk * keys + first + j);
    }
    if (key != kNoFailure) atomicMin(&a.best[p], key);
}

// The leaf of `width` words of a proof over E, bit for bit host_coset_leaf_hash: word 0 at w0, words 1 .. width - 1 from w1 on.  width 1 is an
// f value (vleaf), 2 one value of E, whose components need not be adjacent, 4 and 8 a coset leaf of two or four values, 16 (WIDE only) the
// leaf of a full group at K = 3: its 16 contiguous words as the row leaf of M = 16 (row_vleaf<0>; the field hash takes every width
// through the one chain of row_path_misses, a single trip up to 8 words).  width is the same for every lane of a launch row.
template <int HASH, bool WIDE>
__device__ __forceinline__ Digest ext_vleaf(const uint32_t* pr, uint32_t w0, uint32_t w1, uint32_t width) {
    if constexpr (HASH == 0 && WIDE) {
        if (width == 16u) return row_vleaf<0>(pr + w0, 16u);
    }
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0u;
    v[0] = pr[w0];
    if (width >= 2u) v[1] = pr[w1];
    if constexpr (WIDE) {
        if (width >= 4u) { v[2] = pr[w1 + 1u]; v[3] = pr[w1 + 2u]; }
        if (width >= 8u) {
#pragma unroll
            for (int i = 4; i < 8; ++i) v[i] = pr[w1 + (uint32_t)(i - 1)];
        }
    }
    if constexpr (HASH == 1 && WIDE) {
        uint32_t in[kFhT];
#pragma unroll
        for (int i = 0; i < 8; ++i) { in[i] = v[i]; in[8 + i] = i == 7 ? width : 0u; }
        return fh_row_chain(in, pr + w0, width);
    } else return words_vleaf<HASH>(v, width);
}

// (2) of a proof over E: one lane per proof, blockIdx.y = (query, slot) as in verify_paths_kernel.  Slots 0..2 are the f values, one-word
// leaves.  Every other leaf is the row leaf of the value's words.  One-value leaves: the two words (c0, c1) of the cp tuple, and of opening
// u of group j, which lie at gw + u and gw + s + u; the paths start behind the 2 s value words.  Coset leaves: the 2 s contiguous words of
// the group.  The width is uniform per blockIdx.y, so a wave stays in lockstep.
// The field-hash instance with coset leaves holds the leaf chain of verify_shared_row_paths_kernel<1> and shows the same interleaving: built
// without a second launch bound it takes 132 VGPRs, so it asks for five waves per SIMD as that kernel does.  The other three build at or
// under the counts of verify_paths_kernel without one (a bound of one wave asks for nothing).
template <int HASH, bool COSET>
__global__ void __launch_bounds__(kVerifyThreads, (HASH == 1 && COSET) ? 5 : 1) verify_ext_paths_kernel(VerifyArgs a) {
    const uint32_t p = blockIdx.x * kVerifyThreads + threadIdx.x;
    if (p >= a.count) return;
    const uint32_t slots = COSET ? 3u + a.G : 4u + ((a.G - 1u) << a.K) + (1u << a.ls);
    const uint32_t qk = blockIdx.y / slots, slot = blockIdx.y % slots;
    const uint32_t first = COSET ? 4u : 5u;
    const uint32_t* pr = a.proofs + (size_t)p * a.words;
    const uint32_t tp = query_tp(a, pr, qk);
    const uint32_t fq = a.qbase + qk * a.per_q;
    uint32_t w0, w1, width, path_w, plen, idx, capw, pos;
    if (slot < 3u) {                                      // f(x), f(gx), f(g^2 x) against f's cap
        w0 = w1 = fq + slot * a.t.fwords;
        width = 1u;
        path_w = w0 + 3u;
        plen = a.t.fplen;
        idx = tp + slot * a.B;
        capw = 0u;
        pos = 1u + slot;
    } else if (!COSET && slot == 3u) {                    // cp(x), one value of E, against the cap of group 0's tree
        w0 = fq + 3u * a.t.fwords;
        w1 = w0 + 1u;
        width = 2u;
        path_w = w0 + 4u;
        plen = a.t.cpplen;
        idx = tp;
        capw = a.t.capw[0];
        pos = 4u;
    } else if constexpr (COSET) {                         // the leaf of group j: its s_j component-0 words, then its s_j component-1 words
        const uint32_t j = slot - 3u, steps = group_steps(a, j);
        w0 = fq + a.t.gw[j];
        w1 = w0 + 1u;
        width = 2u << steps;
        path_w = w0 + width + 2u;
        plen = a.t.plen[j];
        idx = tp & ((1u << (a.L - j * a.K - steps)) - 1u);
        capw = a.t.capw[j];
        pos = first + a.G + j;
    } else {                                              // value u of group j at (tp % size + u size / s) % size
        const uint32_t j = (slot - 4u) >> a.K, u = (slot - 4u) & ((1u << a.K) - 1u);
        const uint32_t gs = 1u << group_steps(a, j), gw = fq + a.t.gw[j], size = a.N >> (j * a.K);
        plen = a.t.plen[j];
        w0 = gw + u;
        w1 = gw + gs + u;
        width = 2u;
        path_w = gw + 2u * gs + u * (2u + 8u * plen) + 2u;
        idx = (tp % size + u * (size / gs)) % size;
        capw = a.t.capw[j];
        pos = first + a.G + 8u * j + u;
    }
    if (path_misses<HASH>(ext_vleaf<HASH, COSET>(pr, w0, w1, width), pr + path_w, plen, idx, pr + capw))
        atomicMin(&a.best[p], (int32_t)(qk * (first + (COSET ? 2u : 9u) * a.G) + pos));
}

// (3) of a proof over E (strict only): replay_transcript with two draws per challenge of E and two words per value.
template <bool COSET>
__global__ void __launch_bounds__(kVerifyThreads) verify_ext_transcript_kernel(VerifyArgs a) { replay_transcript<COSET, false, 1>(a); }

std::mutex g_consts_mu;
bool g_consts_done[64] = {false};

hipError_t ensure_verify_consts() {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_consts_mu);
    if (dev < 0 || dev >= 64 || g_consts_done[dev]) return hipSuccess;
    FieldHashConsts c;
    fieldhash_make_consts(c);
    static FieldHashConsts64 c64;
    fieldhash_make_consts64(c, c64);
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_vfh_consts64), &c64, sizeof c64);
    if (e == hipSuccess) g_consts_done[dev] = true;
    return e;
}

// An order key -> the check number verify_proof returns for it: nft f tuples per query (a plain proof: 3; a shared one: 3 per statement,
// or 3 rows) in front of the cp tuple and the groups.
int32_t order_key_to_check(int32_t key, uint32_t nft, uint32_t G, bool coset) {
    const uint32_t first = nft + (coset ? 1u : 2u), pos = (uint32_t)key % (first + (coset ? 2u : 9u) * G);
    if (pos == 0) return -2;
    if (pos <= nft) return -(int32_t)(4u + (pos - 1u) % 3u);   // -4 .. -6 of statement (pos - 1) / 3, or of row pos - 1
    if (pos < first) return -7;                           // one-value leaves only
    if (pos < first + G) return -(int32_t)(100u + (pos - first));
    if (coset) return -(int32_t)(300u + (pos - first - G));
    const uint32_t j = (pos - first - G) / 8u, t = (pos - first - G) % 8u;
    return -(int32_t)((t ? 400u : 300u) + j);
}

}  // namespace
}  // namespace zk

struct zk_verifier {
    int device = 0;
    zk::ProofFormat fmt;                               // the format of the proofs (transcript.hpp), one field per setter
    int hash = ZK_HASH_SHA256;
    hipStream_t stream = nullptr, tstream = nullptr;   // paths + algebra; transcript (runs beside them)
    hipEvent_t ev_in = nullptr, ev_t = nullptr;
    uint8_t* d_buf = nullptr;                          // proofs, public_last, states, then the three per-proof results
    uint8_t* h_in = nullptr;                           // pinned staging of the inputs
    int32_t* h_out = nullptr;                          // pinned: best, malformed, tcode
    size_t cap = 0, cap_in = 0, cap_out = 0;           // proofs the buffers hold
};

namespace {

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// pub: the bytes of a proof's public values, 4 per statement
int verifier_reserve(zk_verifier* v, size_t chunk, size_t len, size_t pub) {
    const size_t in_bytes = chunk * (len + pub + 32);
    const size_t dev_bytes = align256(chunk * len) + align256(chunk * pub) + align256(chunk * 32) + 3 * align256(chunk * 4);
    if (chunk <= v->cap && in_bytes <= v->cap_in && dev_bytes <= v->cap_out) return ZK_OK;
    HIPCHK(hipStreamSynchronize(v->stream));
    HIPCHK(hipStreamSynchronize(v->tstream));
    if (v->d_buf) (void)hipFree(v->d_buf);
    if (v->h_in) (void)hipHostFree(v->h_in);
    if (v->h_out) (void)hipHostFree(v->h_out);
    v->d_buf = nullptr; v->h_in = nullptr; v->h_out = nullptr; v->cap = v->cap_in = v->cap_out = 0;
    if (hipMalloc((void**)&v->d_buf, dev_bytes) != hipSuccess) return fail(ZK_ERR_NOMEM, "zk_verifier_run: hipMalloc(%zu) failed", dev_bytes);
    if (hipHostMalloc((void**)&v->h_in, in_bytes) != hipSuccess) return fail(ZK_ERR_NOMEM, "zk_verifier_run: hipHostMalloc(%zu) failed", in_bytes);
    if (hipHostMalloc((void**)&v->h_out, chunk * 12) != hipSuccess) return fail(ZK_ERR_NOMEM, "zk_verifier_run: hipHostMalloc(%zu) failed", chunk * 12);
    v->cap = chunk; v->cap_in = in_bytes; v->cap_out = dev_bytes;
    return ZK_OK;
}

// One chunk of proofs: stage, copy in, three kernels, copy the per-proof results out, decide each proof.
int verifier_chunk(zk_verifier* v, const uint8_t* proofs, size_t stride, size_t count, const uint8_t* states, const uint32_t* public_last,
                   int32_t* checks_out, size_t len) {
    const ProofFormat& f = v->fmt;
    const uint32_t log_n = f.log_n, log_b = f.log_b, q = f.q, D = f.stop, L = f.L();
    const uint32_t R = f.rounds(), K = f.fold, G = f.groups();   // the folded rounds (early stop: R', and G' groups)
    const bool coset = f.coset, shared = f.lb != 0, ext = f.ext != 0;   // ProofFormat::ok(): never shared and ext
    const size_t pub = (size_t)4 << f.lb;                  // bytes of a proof's public values
    // inputs: [count][len] proofs, [count][2^lb] public_last, [count][32] states, packed into the pinned staging buffer
    uint8_t* hp = v->h_in;
    if (stride == len) memcpy(hp, proofs, count * len);
    else for (size_t i = 0; i < count; ++i) memcpy(hp + i * len, proofs + i * stride, len);
    memcpy(hp + count * len, public_last, count * pub);
    if (states) memcpy(hp + count * len + count * pub, states, count * 32);
    uint8_t* d = v->d_buf;
    uint8_t* d_pub = d + align256(count * len);
    uint8_t* d_states = d_pub + align256(count * pub);
    uint8_t* d_res = d_states + align256(count * 32);
    VerifyArgs a{};
    a.proofs = reinterpret_cast<const uint32_t*>(d);
    a.pub = reinterpret_cast<const uint32_t*>(d_pub);
    a.states = reinterpret_cast<const uint32_t*>(d_states);
    a.best = reinterpret_cast<int32_t*>(d_res);
    a.malformed = reinterpret_cast<uint32_t*>(d_res + align256(count * 4));
    a.tcode = reinterpret_cast<int32_t*>(d_res + 2 * align256(count * 4));
    a.count = (uint32_t)count; a.words = (uint32_t)(len / 4); a.q = q; a.R = R; a.L = L;
    a.B = 1u << log_b; a.N = 1u << L; a.log_n = log_n;
    a.h = root_of_unity(L);
    const uint32_t g = root_of_unity(log_n);
    a.gm1 = invmod(g); a.gm2 = mulmod(a.gm1, a.gm1); a.gm3 = mulmod(a.gm2, a.gm1);
    a.gw = f.grind ? 2u : 0u;
    a.gmask = f.grind ? ~0u << (32u - f.grind) : 0u;
    a.D = D;
    a.K = K; a.G = G; a.ls = f.steps(G - 1u);
    // Where the fields sit, in words, from one pass over the header and one over a query (transcript.hpp): ProofLayout
    if (G + 1u > kLayoutTrees) return fail(ZK_ERR_STATE, "zk_verifier_run: more than %u trees", kLayoutTrees);
    uint32_t w = 0;
    f.for_each_head([&](ProofFormat::Head what, uint32_t j, size_t bytes) {
        switch (what) {
            case ProofFormat::kFTree: a.t.fcapn = (uint32_t)(bytes / 4); break;
            case ProofFormat::kAlphas: a.t.aw = w; break;
            case ProofFormat::kTree: a.t.capw[j] = w; a.t.capn[j] = (uint32_t)(bytes / 4); break;
            case ProofFormat::kBeta: a.t.bw[j] = w; break;
            case ProofFormat::kFinal: a.t.ftw = w; break;
            case ProofFormat::kNonce: case ProofFormat::kRaws: break;
        }
        w += (uint32_t)(bytes / 4);
        return true;
    });
    a.qbase = w;
    a.t.fplen = (uint32_t)f.f_path();
    a.t.fwords = (uint32_t)(Channel::group_bytes(f.rows ? (size_t)1 << f.lb : 1, a.t.fplen, f.rows) / 4);   // 3 + 8 fplen, or a row's 2^lb + 2 + 8 fplen
    a.t.cpplen = (uint32_t)f.tree_path(0);
    a.t.lb = f.lb; a.t.ext = f.ext; a.t.nft = f.rows ? 3u : 3u << f.lb; a.t.fshare = f.rows ? 0u : 8u << f.f_cap();
    a.t.keys = a.t.nft + (coset ? 1u + 2u * G : 2u + 9u * G);
    const uint32_t nf = a.t.nft + (coset ? 0u : 1u);         // the tuples in front of group 0: the f tuples and, with one-value leaves, cp(x)
    uint32_t tuple = 0, off = 0;
    f.for_each_tuple([&](size_t s, size_t plen, bool one_leaf, uint32_t words) {   // words per value: 2 for cp and the groups of an ext proof
        const uint32_t tw = (uint32_t)(ProofFormat::tuple_bytes(s, plen, one_leaf, words) / 4);
        if (tuple >= nf) { a.t.plen[tuple - nf] = (uint32_t)plen; a.t.gw[tuple - nf] = off; }
        else if (tuple == a.t.nft) a.t.cpwords = tw;       // one-value leaves: 2 + words + 8 cpplen
        off += tw;
        ++tuple;
    });
    a.per_q = off;
    if (a.qbase + (size_t)q * a.per_q != len / 4) return fail(ZK_ERR_STATE, "zk_verifier_run: the layout does not add up to the proof length");
    const uint32_t w8 = invmod(powmod(a.h, (uint64_t)a.N >> 3));
    a.inv2m = to_mont(invmod(2)); a.wm1 = to_mont(w8); a.wm2 = to_mont(mulmod(w8, w8)); a.wm3 = to_mont(mulmod(mulmod(w8, w8), w8));

    HIPCHK(hipMemcpyAsync(d, hp, count * len, hipMemcpyHostToDevice, v->stream));
    HIPCHK(hipMemcpyAsync(d_pub, hp + count * len, count * pub, hipMemcpyHostToDevice, v->stream));
    if (states) HIPCHK(hipMemcpyAsync(d_states, hp + count * len + count * pub, count * 32, hipMemcpyHostToDevice, v->stream));
    HIPCHK(hipMemsetAsync(a.best, 0x7f, count * 4, v->stream));
    HIPCHK(hipMemsetAsync(a.malformed, 0, count * 4, v->stream));
    HIPCHK(hipMemsetAsync(a.tcode, 0, count * 4, v->stream));
    const uint32_t gx = (uint32_t)((count + kVerifyThreads - 1) / kVerifyThreads);
    if (states) {                                      // the transcript chains run beside the paths: cost = max of the two
        HIPCHK(hipEventRecord(v->ev_in, v->stream));
        HIPCHK(hipStreamWaitEvent(v->tstream, v->ev_in, 0));
        if (shared) {
            if (coset) hipLaunchKernelGGL(verify_shared_transcript_kernel<true>, dim3(gx), dim3(kVerifyThreads), 0, v->tstream, a);
            else hipLaunchKernelGGL(verify_shared_transcript_kernel<false>, dim3(gx), dim3(kVerifyThreads), 0, v->tstream, a);
        } else if (ext) {
            if (coset) hipLaunchKernelGGL(verify_ext_transcript_kernel<true>, dim3(gx), dim3(kVerifyThreads), 0, v->tstream, a);
            else hipLaunchKernelGGL(verify_ext_transcript_kernel<false>, dim3(gx), dim3(kVerifyThreads), 0, v->tstream, a);
        } else if (coset) hipLaunchKernelGGL(verify_transcript_kernel<true>, dim3(gx), dim3(kVerifyThreads), 0, v->tstream, a);
        else hipLaunchKernelGGL(verify_transcript_kernel<false>, dim3(gx), dim3(kVerifyThreads), 0, v->tstream, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(v->ev_t, v->tstream));
    }
    const uint64_t lanes = (uint64_t)count * q;
    const dim3 agrid((uint32_t)((lanes + kVerifyThreads - 1) / kVerifyThreads));
    if (shared) {
        if (coset) {
            if (f.rows) hipLaunchKernelGGL((verify_shared_algebra_kernel<true, true>), agrid, dim3(kVerifyThreads), 0, v->stream, a);
            else hipLaunchKernelGGL((verify_shared_algebra_kernel<true, false>), agrid, dim3(kVerifyThreads), 0, v->stream, a);
        } else if (f.rows) hipLaunchKernelGGL((verify_shared_algebra_kernel<false, true>), agrid, dim3(kVerifyThreads), 0, v->stream, a);
        else hipLaunchKernelGGL((verify_shared_algebra_kernel<false, false>), agrid, dim3(kVerifyThreads), 0, v->stream, a);
    } else if (ext) {
        if (coset) hipLaunchKernelGGL(verify_ext_algebra_kernel<true>, agrid, dim3(kVerifyThreads), 0, v->stream, a);
        else hipLaunchKernelGGL(verify_ext_algebra_kernel<false>, agrid, dim3(kVerifyThreads), 0, v->stream, a);
    } else if (coset) hipLaunchKernelGGL(verify_algebra_kernel<true>, agrid, dim3(kVerifyThreads), 0, v->stream, a);   // one instance per leaf format covers every K and D
    else hipLaunchKernelGGL(verify_algebra_kernel<false>, agrid, dim3(kVerifyThreads), 0, v->stream, a);
    HIPCHK(hipGetLastError());
    const bool sha = v->hash == ZK_HASH_SHA256;
    if (shared) {
        // the f tuples: three rows per query with the proof on the lane, or 3 * 2^lb tuples with the (proof, statement) on the lane
        if (f.rows) {
            const dim3 fgrid(gx, 3u * q);
            if (sha) hipLaunchKernelGGL(verify_shared_row_paths_kernel<0>, fgrid, dim3(kVerifyThreads), 0, v->stream, a);
            else hipLaunchKernelGGL(verify_shared_row_paths_kernel<1>, fgrid, dim3(kVerifyThreads), 0, v->stream, a);
        } else {
            const dim3 fgrid((uint32_t)((((uint64_t)count << f.lb) + kVerifyThreads - 1) / kVerifyThreads), 3u * q);
            if (sha) hipLaunchKernelGGL(verify_shared_f_paths_kernel<0>, fgrid, dim3(kVerifyThreads), 0, v->stream, a);
            else hipLaunchKernelGGL(verify_shared_f_paths_kernel<1>, fgrid, dim3(kVerifyThreads), 0, v->stream, a);
        }
        HIPCHK(hipGetLastError());
        const dim3 pgrid(gx, q * (coset ? G : 1u + ((G - 1u) << K) + (1u << a.ls)));   // the cp tuple and the groups
        if (coset) {
            if (sha) hipLaunchKernelGGL((verify_shared_paths_kernel<0, true>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
            else hipLaunchKernelGGL((verify_shared_paths_kernel<1, true>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
        } else if (sha) hipLaunchKernelGGL((verify_shared_paths_kernel<0, false>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
        else hipLaunchKernelGGL((verify_shared_paths_kernel<1, false>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
    } else {
        const dim3 pgrid(gx, q * (coset ? 3u + G : 4u + ((G - 1u) << K) + (1u << a.ls)));
        if (ext) {                                         // the same slots, leaves of the values' words
            if (coset) {
                if (sha) hipLaunchKernelGGL((verify_ext_paths_kernel<0, true>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
                else hipLaunchKernelGGL((verify_ext_paths_kernel<1, true>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
            } else if (sha) hipLaunchKernelGGL((verify_ext_paths_kernel<0, false>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
            else hipLaunchKernelGGL((verify_ext_paths_kernel<1, false>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
        } else if (coset) {
            if (sha) hipLaunchKernelGGL((verify_paths_kernel<0, true>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
            else hipLaunchKernelGGL((verify_paths_kernel<1, true>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
        } else if (sha) hipLaunchKernelGGL((verify_paths_kernel<0, false>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
        else hipLaunchKernelGGL((verify_paths_kernel<1, false>), pgrid, dim3(kVerifyThreads), 0, v->stream, a);
    }
    HIPCHK(hipGetLastError());
    if (states) HIPCHK(hipStreamWaitEvent(v->stream, v->ev_t, 0));
    HIPCHK(hipMemcpyAsync(v->h_out, a.best, count * 4, hipMemcpyDeviceToHost, v->stream));
    HIPCHK(hipMemcpyAsync(v->h_out + count, a.malformed, count * 4, hipMemcpyDeviceToHost, v->stream));
    HIPCHK(hipMemcpyAsync(v->h_out + 2 * count, a.tcode, count * 4, hipMemcpyDeviceToHost, v->stream));
    HIPCHK(hipStreamSynchronize(v->stream));
    const int32_t* best = v->h_out;
    const int32_t* malformed = v->h_out + count;
    const int32_t* tcode = v->h_out + 2 * count;
    for (size_t i = 0; i < count; ++i) {
        int32_t c;
        if (states && tcode[i]) c = tcode[i];
        else if (malformed[i])                             // garbage only
            c = verify_proof(proofs + i * stride, len, f, public_last + (i << f.lb), v->hash);
        else if (best[i] == kNoFailure) c = 0;
        else c = order_key_to_check(best[i], a.t.nft, G, coset);
        checks_out[i] = c;
    }
    return ZK_OK;
}

}  // namespace

extern "C" {

int zk_verifier_destroy(zk_verifier* v) {
    if (!v) return ZK_OK;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    if (v->tstream) (void)hipStreamSynchronize(v->tstream);
    if (v->d_buf) (void)hipFree(v->d_buf);
    if (v->h_in) (void)hipHostFree(v->h_in);
    if (v->h_out) (void)hipHostFree(v->h_out);
    if (v->ev_in) (void)hipEventDestroy(v->ev_in);
    if (v->ev_t) (void)hipEventDestroy(v->ev_t);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    if (v->tstream) (void)hipStreamDestroy(v->tstream);
    delete v;
    return ZK_OK;
}

int zk_verifier_create(int device, uint32_t log_n, uint32_t log_b, zk_verifier** out) {
    if (!out) return fail(ZK_ERR_INVALID, "zk_verifier_create: out is null");
    *out = nullptr;
    // the sizes verify_proof accepts (it answers -1 to any other)
    if (log_n < 2 || log_b < 1 || log_n + log_b > 30)
        return fail(ZK_ERR_INVALID, "zk_verifier_create: need 2 <= log_n, 1 <= log_blowup, log_n + log_blowup <= 30 (got %u, %u)", log_n, log_b);
    HIPCHK(hipSetDevice(device));
    zk_verifier* v = new (std::nothrow) zk_verifier();
    if (!v) return fail(ZK_ERR_NOMEM, "out of host memory");
    v->device = device; v->fmt.log_n = log_n; v->fmt.log_b = log_b;
    hipError_t e = hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&v->tstream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&v->ev_in, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&v->ev_t, hipEventDisableTiming);
    if (e == hipSuccess) e = ensure_verify_consts();
    if (e != hipSuccess) {
        zk_verifier_destroy(v);
        return fail(ZK_ERR_HIP, "zk_verifier_create: %s", hipGetErrorString(e));
    }
    *out = v;
    return ZK_OK;
}

int zk_verifier_set_queries(zk_verifier* v, uint32_t n_queries) {
    if (!v) return fail(ZK_ERR_INVALID, "null verifier");
    if (n_queries < 1 || n_queries > kMaxQueries) return fail(ZK_ERR_INVALID, "zk_verifier_set_queries: need 1 <= n_queries <= %u", kMaxQueries);
    v->fmt.q = n_queries;
    return ZK_OK;
}

int zk_verifier_set_grinding(zk_verifier* v, uint32_t grind_bits) {
    if (!v) return fail(ZK_ERR_INVALID, "null verifier");
    if (grind_bits > kMaxGrindBits) return fail(ZK_ERR_INVALID, "zk_verifier_set_grinding: need grind_bits <= %u (got %u)", kMaxGrindBits, grind_bits);
    v->fmt.grind = grind_bits;
    return ZK_OK;
}

int zk_verifier_set_hash(zk_verifier* v, int hash_kind) {
    // refused before the handle is looked at: no setting of this class takes it
    if (hash_kind == ZK_HASH_BLAKE2S) return fail(ZK_ERR_INVALID, "zk_verifier_set_hash: BLAKE2s (hash 2) is not built for this entry point yet");
    if (!v) return fail(ZK_ERR_INVALID, "null verifier");
    if (hash_kind != ZK_HASH_SHA256 && hash_kind != ZK_HASH_FIELD) return fail(ZK_ERR_INVALID, "zk_verifier_set_hash: unknown hash %d", hash_kind);
    v->hash = hash_kind;
    return ZK_OK;
}

int zk_verifier_set_fold(zk_verifier* v, uint32_t fold_log) {
    if (!v) return fail(ZK_ERR_INVALID, "null verifier");
    if (fold_log < 1 || fold_log > kMaxFoldLog) return fail(ZK_ERR_INVALID, "zk_verifier_set_fold: need 1 <= fold_log <= %u (got %u)", kMaxFoldLog, fold_log);
    v->fmt.fold = fold_log;
    return ZK_OK;
}

uint32_t zk_verifier_get_fold(const zk_verifier* v) { return v ? v->fmt.fold : 0u; }

int zk_verifier_set_fri_stop(zk_verifier* v, uint32_t stop_log) {
    if (!v) return fail(ZK_ERR_INVALID, "null verifier");
    if (!stop_ok(v->fmt.log_n, v->fmt.log_b, stop_log))
        return fail(ZK_ERR_INVALID, "zk_verifier_set_fri_stop: need stop_log 0, or 1 <= stop_log <= %u with stop_log <= log_n - 1 and stop_log + log_blowup <= %u (got %u for %u, %u)",
                    kMaxStopLog, kMaxStopLayerLog, stop_log, v->fmt.log_n, v->fmt.log_b);
    v->fmt.stop = stop_log;
    return ZK_OK;
}

uint32_t zk_verifier_get_fri_stop(const zk_verifier* v) { return v ? v->fmt.stop : 0u; }

int zk_verifier_set_merkle_cap(zk_verifier* v, uint32_t cap_log) {
    if (!v) return fail(ZK_ERR_INVALID, "null verifier");
    if (cap_log > kMaxCapLog) return fail(ZK_ERR_INVALID, "zk_verifier_set_merkle_cap: need cap_log <= %u (got %u)", kMaxCapLog, cap_log);
    v->fmt.cap = cap_log;
    return ZK_OK;
}

uint32_t zk_verifier_get_merkle_cap(const zk_verifier* v) { return v ? v->fmt.cap : 0u; }

int zk_verifier_set_coset_leaves(zk_verifier* v, int on) {
    if (!v) return fail(ZK_ERR_INVALID, "null verifier");
    v->fmt.coset = on != 0;
    return ZK_OK;
}

int zk_verifier_set_ext(zk_verifier* v, uint32_t ext_log) {
    if (!v) return fail(ZK_ERR_INVALID, "null verifier");
    if (ext_log > 1) return fail(ZK_ERR_INVALID, "zk_verifier_set_ext: need ext_log 0 or 1 (got %u; 2, the quartic extension, is reserved)", ext_log);
    if (ext_log && v->fmt.lb) return fail(ZK_ERR_INVALID, "zk_verifier_set_ext: shared proofs (zk_verifier_set_shared, log_batch %u) have no ext format", v->fmt.lb);
    v->fmt.ext = ext_log;
    return ZK_OK;
}

uint32_t zk_verifier_get_ext(const zk_verifier* v) { return v ? v->fmt.ext : 0u; }

int zk_verifier_get_coset_leaves(const zk_verifier* v) { return v && v->fmt.coset ? 1 : 0; }

int zk_verifier_set_shared(zk_verifier* v, uint32_t log_batch, int row_leaves) {
    if (!v) return fail(ZK_ERR_INVALID, "null verifier");
    if (log_batch > kMaxSharedLog) return fail(ZK_ERR_INVALID, "zk_verifier_set_shared: need log_batch <= %u (got %u)", kMaxSharedLog, log_batch);
    if (row_leaves && log_batch < 1) return fail(ZK_ERR_INVALID, "zk_verifier_set_shared: row leaves need log_batch >= 1");
    if (log_batch && v->fmt.ext) return fail(ZK_ERR_INVALID, "zk_verifier_set_shared: proofs over E (zk_verifier_set_ext, ext_log %u) are not shared", v->fmt.ext);
    v->fmt.lb = log_batch;
    v->fmt.rows = row_leaves != 0;
    return ZK_OK;
}

uint32_t zk_verifier_get_shared(const zk_verifier* v) { return v ? v->fmt.lb : 0u; }

int zk_verifier_get_shared_rows(const zk_verifier* v) { return v && v->fmt.rows ? 1 : 0; }

int zk_verifier_run(zk_verifier* v, const uint8_t* proofs, size_t stride, size_t count, const uint8_t* states, const uint32_t* public_last,
                    int32_t* checks_out) {
    if (!v) return fail(ZK_ERR_INVALID, "null verifier");
    if (count == 0) return ZK_OK;
    if (!proofs || !public_last || !checks_out) return fail(ZK_ERR_INVALID, "zk_verifier_run: null argument");
    const size_t len = v->fmt.data_len();
    if (stride < len) return fail(ZK_ERR_INVALID, "zk_verifier_run: stride %zu < proof length %zu", stride, len);
    if (count > SIZE_MAX / stride) return fail(ZK_ERR_INVALID, "zk_verifier_run: count * stride overflows");
    HIPCHK(hipSetDevice(v->device));
    // chunks of at most 2^16 proofs and ~256 MiB of proof bytes bound the staging and device buffers
    size_t chunk = ((size_t)256 << 20) / len;
    if (chunk > 65536) chunk = 65536;
    if (chunk < 1) chunk = 1;
    if (chunk > count) chunk = count;
    const uint32_t lb = v->fmt.lb;                      // public_last: [count][2^lb], statement-major per proof
    if (int rc = verifier_reserve(v, chunk, len, (size_t)4 << lb)) return rc;
    for (size_t i = 0; i < count; i += chunk) {
        const size_t c = count - i < chunk ? count - i : chunk;
        if (int rc = verifier_chunk(v, proofs + i * stride, stride, c, states ? states + 32 * i : nullptr, public_last + (i << lb), checks_out + i, len))
            return rc;
    }
    for (size_t i = 0; i < count; ++i)
        if (checks_out[i]) return fail(ZK_ERR_VERIFY, "zk_verifier_run: proof %zu rejected at check %d", i, checks_out[i]);
    return ZK_OK;
}

}  // extern "C"
