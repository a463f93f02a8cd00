// batch.hip -- batched proving: 2^log_batch proofs of one size in lockstep (zk_batch_*).
//
// prover.rs:9-293 is run for every proof of the batch with the SAME kernels as one proof on a domain
// batch times larger: layer l is stored proof-major ([batch][m_l]), so the trees of the batch are the
// bottom of one heap over batch*m_l leaves whose nodes of depth log_batch are the per-proof roots.
// The device posts those (MailArgs.top = log_batch), each proof's own channel absorbs its root and
// draws its own challenges (host threads), and the next launch reads them from a per-proof table.
// One loop over the groups of `fold` rounds serves every folding factor (K = 1: one round per group, fold fused into the leaf
// hashing); the openings and their encoding are transcript.hpp's for_each_opening and Channel::commit_group.
// ONE pipeline makes every proof (struct Run and run_commit_f, run_groups, run_queries, run_decommit below): a run has a number of
// channels and the widths of its two stages, log2 of the trees a launch builds side by side.  zk_batch_prove is the run with 2^lb channels
// at width lb; a shared proof (zk_batch_prove_shared: one proof over the sum of the batch's compositions) is the run with ONE channel whose
// FRI stage has width 0 and whose f stage has width lb, or 0 with row leaves.  The entry points differ in how tree 0 is committed, how the
// alphas are drawn and how cp is made, and in nothing after that: a new format setting is written into the pipeline once.
// Coset leaves (zk_batch_set_coset_leaves): the tree over a group's input layer has one leaf per opened coset, so proof p's tree over
// len values has m = len / s leaves and the batch heap batch * m; cp is composed by its own launch, every K folds with the batched
// multi-fold, and the trees come from launch_merkle_build_coset_batch -- prove_resident / prove_fold_rounds (zkstark.hip) per proof.
// Early stop (zk_batch_set_fri_stop, D > 0): the groups are those of the first R' = log_n - D rounds, every K folds with the batched
// multi-fold, the last group's output (layer 1 + R' of the batch) gets no tree; one launch of fri_final_poly_batch_kernel turns it into
// the compact [batch][1 + 2^D] table (count, coefficients) and each proof's channel commits its own 4 * 2^D bytes -- prove_finish per proof.
// Challenges in E (zk_batch_set_ext): the layers >= 1 are two planes [batch][m_l] each, the component-1 halves of every
// proof's challenges sit in a table beside BatchChal, cp comes from one launch of compose_ext_batch_kernel, every K and leaf format takes
// the grouped loop with the batched butterfly over E, the trees are the row tree over the two planes (one-value leaves) or come from
// launch_merkle_build_coset_ext_batch, and a query gathers the component-0 slots of a leaf, then its component-1 slots --
// prove_ext_rounds / prove_finish (zkstark.hip) per proof.  zk_batch_prove only: a shared proof has no ext format.
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "host_sha.hpp"
#include "internal.hpp"
#include "pool.hpp"
#include "sha256.hpp"
#include "transcript.hpp"

using namespace zk;
using namespace zk::impl;

struct zk_batch {
    int device = 0;
    std::atomic<bool> busy{false};    // a zk_batch_prove is running: the setters refuse to change the batch under it
    uint32_t log_n = 0, log_b = 0, lb = 0, L = 0, R = 0;
    size_t n = 0, N = 0, B = 0, batch = 0;
    hipStream_t stream = nullptr;
    zk_dom* dom = nullptr;
    uint32_t* d_trace = nullptr;      // [batch][n]: a[0..n-2], 0
    uint32_t* d_coef = nullptr;       // [batch][2n]
    uint32_t* d_layers = nullptr;     // layer l: [batch][m_l]
    uint32_t* d_trees = nullptr;      // tree l: heap over batch*m_l leaves
    uint32_t* d_seed = nullptr;       // [2][batch] seeds of zk_batch_gen_fibsq
    std::vector<size_t> layer_off, tree_off;
    BatchChal* h_chal = nullptr;      // pinned
    BatchChal* d_chal = nullptr;
    uint32_t* h_mail = nullptr;       // pinned, mapped (MailArgs layout)
    uint32_t* d_mail = nullptr;
    uint32_t* d_counter = nullptr;
    bool counters_dirty = false;
    uint32_t mail_seq = 0;
    uint64_t *d_goff = nullptr, *h_goff = nullptr;
    uint32_t *d_gout = nullptr, *h_gout = nullptr;
    uint32_t* h_last = nullptr;       // pinned: [batch][B] last layer / [batch] last trace values
    size_t per_proof_vals = 0, per_proof_digs = 0;   // per query
    // The format of the next zk_batch_prove (transcript.hpp), one field per setter: q (1 = the reference, prover.rs:263), grind, fold
    // (1 = the reference), coset, stop (0 = fold down to a constant, the reference) and cap
    ProofFormat fmt;
    uint32_t proved_fold = 1, proved_stop = 0;   // ... of the last zk_batch_prove, whose skipped_trees these are:
    int proved_hash = 0;              // ... and the Merkle hash its trees were built with (zk_batch_merkle_nodes hashes the levels above the roots)
    uint64_t skipped_trees = 0;       // bit id: that proof built no tree (and no layer) `id`
    uint32_t* d_work = nullptr;       // [batch][8] per-proof constants of the multi-fold (allocated by the first fold > 1, coset leaves or early stop)
    uint32_t *d_final = nullptr, *h_final = nullptr;   // [batch][1 + 2^stop]: count of high coefficients, final polynomial (stop > 0; h_: pinned)
    uint8_t tree_steps[34] = {0};     // tree id of the last zk_batch_prove: its leaves hold 2^tree_steps values (0: one-value leaves)
    // Merkle caps (transcript.hpp): every proof commits the 2^ce digests of depth ce = min(cap, lg - 1) of each of
    // its trees, i.e. the batch heap is built down to depth lb + ce and nothing above is hashed.  tree_cap[t]: the ce of tree t in the
    // last zk_batch_prove.  h_cap / d_cap: pinned, mapped, 16 + 8 * 2^(lb + ce of the f tree) words in the mailbox's layout, for the
    // hand-overs the mailbox cannot hold (lb + ce > kMaxHostLog); allocated by the setter only when the f tree needs it.
    uint8_t tree_cap[34] = {0};
    bool proved = false;              // a zk_batch_prove has run: tree_cap, tree_steps and skipped_trees describe it
    bool shared_rows = false;         // the next zk_batch_prove_shared commits f as row leaves (zk_batch_set_shared_rows)
    bool rows_tree0 = false;          // the last proof was one: tree 0 holds the tree over the rows, not the batch's f heap
    uint32_t *h_cap = nullptr, *d_cap = nullptr;
    size_t cap_words = 0;
    Grinder* grinder = nullptr;       // one launch grinds for every proof of the batch (created by the setter above kGrindHostMaxBits)
    int hash = 0;                    // Merkle hash: 0 = SHA-256 (reference), 1 = field-native
    std::vector<uint32_t> first, last;
    bool have_traces = false;
    size_t device_bytes = 0;
    Pool* pool = nullptr;
    // small batches: the device stops each tree `extra` levels above the per-proof roots and the host threads
    // hash those levels (host_sha.hpp); staged level-major like the batch heap, copied back by scatter_kernel
    bool host_levels = false;
    uint32_t* h_stage = nullptr;      // pinned, mapped
    uint32_t* d_stage = nullptr;
    size_t stage_words = 0, stage_used = 0;
    ScatterSeg* h_segs = nullptr;
    ScatterSeg* d_segs = nullptr;
    uint32_t n_segs = 0;
    double seg_words = 0;
    // A batch of ONE proof is a single proof: it runs on the one-call prover (zk_prove_resident: fused host tail,
    // no per-round challenge table), so the smallest batch is never slower than zk_prove.
    zk_ctx* single = nullptr;
    std::vector<uint32_t> single_trace;
    // Challenges in E (zk_batch_set_ext; transcript.hpp "ext").  With fmt.ext = 1 layer id >= 1 is two planes, component 0
    // first, each the proof-major [batch][m_l] layer above; they lie behind the base layers in d_layers, from word ext_base on (the setter
    // sizes d_layers both ways, as zk_ctx_set_ext does).  layer_words: the base layers.  xchal: the component-1 halves of every proof's
    // challenges beside its BatchChal row; d_xwork: [batch][kFoldExtRow] constants of E of the group fold; h_xlast: plane 1 of the last
    // layer, [batch][B], behind h_xchal in one pinned block.  All four exist only while ext is on.
    size_t layer_words = 0, ext_base = 0;
    BatchChalExt *h_xchal = nullptr, *d_xchal = nullptr;
    uint32_t *d_xwork = nullptr, *h_xlast = nullptr;
};

namespace {

size_t blayer_size(const zk_batch* b, uint32_t layer) { return layer == 0 ? b->N : (b->N >> (layer - 1)); }
uint32_t blayer_log(const zk_batch* b, uint32_t layer) { return layer == 0 ? b->L : b->L - (layer - 1); }
// Layer id >= 1 of an ext batch: two planes of batch * m_l words, component 0 first
size_t bext_off(const zk_batch* b, uint32_t id) { return b->ext_base + 2 * (b->layer_off[id] - b->layer_off[1]); }
uint32_t* bext_layer(zk_batch* b, uint32_t id) { return b->d_layers + bext_off(b, id); }

// Levels of each proof's tree (over 2^log_m leaves) that the host hashes: as many as the mailbox holds
// (2^kMaxHostLog digests for the whole batch), none for the field hash or without SHA extensions.
// lb, here and in the helpers below: the width of the stage, log2 of the trees built side by side -- b->lb for zk_batch_prove and the f
// tree of a shared proof, 0 for the one FRI of a shared proof (zk_batch_prove_shared), which uses proof 0's share of every layer and heap.
uint32_t bextra(const zk_batch* b, uint32_t log_m, uint32_t lb) {
    if (!b->host_levels || b->hash != 0 || lb >= kMaxHostLog || log_m < 2) return 0;
    uint32_t h = kMaxHostLog - lb;
    if (h > 8) h = 8;                                    // <= 255 nodes per proof on one thread (~8 us), as the single prover
    if (h > log_m - 1) h = log_m - 1;
    return h >= 3 ? h : 0;                               // two levels are not worth a hand-over
}
// How the build of a tree whose proofs commit it at depth ce (0: their roots) reaches the host.  Through the mailbox at depth
// lb + max(ce, host share) of the batch heap when that fits (ce = 0: what it always was); the host then hashes from its share down
// to ce (h levels, 0 when the cap is at or below the share).  Otherwise the host's share is dropped: the build ends at depth lb + ce
// without a mailbox and launch_digest_level_post copies that level into h_cap.  top: the depth the build ends at.
struct Hand { uint32_t top, h; bool mailbox; };
Hand bhand(const zk_batch* b, uint32_t ce, uint32_t log_m, uint32_t lb) {
    const uint32_t h = bextra(b, log_m, lb), deep = h > ce ? h : ce;
    if (lb + deep <= kMaxHostLog) return Hand{lb + deep, h > ce ? h : 0, true};
    return Hand{lb + ce, 0, false};
}
// cap > 0: the 16 + 8 * 2^(lb + ce) words of h_cap when the f tree (the deepest cap of a proof) does not fit the mailbox, else 0
size_t bcap_words(const zk_batch* b, const ProofFormat& f) {
    const uint32_t e = b->lb + f.f_cap();
    return f.cap && e > kMaxHostLog ? kMailDigests + ((size_t)8 << e) : 0;
}
// Hand-over of the commit launch of `tree` (2^log_m leaves per proof): records the depth its proofs commit it at.
MailArgs bmail(zk_batch* b, uint32_t tree, uint32_t log_m, uint32_t lb) {
    MailArgs m;
    if (b->counters_dirty) { (void)hipMemsetAsync(b->d_counter, 0, 64, b->stream); b->counters_dirty = false; }
    const uint32_t ce = b->fmt.cap ? cap_eff(b->fmt.cap, log_m) : 0;
    const Hand hd = bhand(b, ce, log_m, lb);
    b->tree_cap[tree] = (uint8_t)ce;
    m.seq = ++b->mail_seq; m.top = hd.top;
    if (hd.mailbox) { m.mailbox = b->d_mail; m.counter = b->d_counter; }   // else: no mailbox, no continuation; bpost follows the build
    return m;
}
// Behind the build of `tree`: a cap deeper than the mailbox holds is posted by a launch of its own (the flag is the mailbox's).
int bpost(zk_batch* b, uint32_t tree, uint32_t log_m, uint32_t lb) {
    const Hand hd = bhand(b, b->tree_cap[tree], log_m, lb);
    if (hd.mailbox) return ZK_OK;
    if (!b->h_cap || kMailDigests + ((size_t)8 << hd.top) > b->cap_words) return fail(ZK_ERR_STATE, "zk_batch_prove: no buffer for a cap of 2^%u digests", hd.top);
    HIPCHK(launch_digest_level_post(b->d_trees + b->tree_off[tree], hd.top, b->d_cap + kMailDigests, b->d_mail, b->mail_seq, b->d_counter, b->stream, nullptr));
    return ZK_OK;
}
// Proof-of-work nonce of every proof after its free term (DESIGN.md "Grinding"), committed to its channel: one thread per proof for
// small g, else one launch per chunk for all proofs still searching.
int bgrind(zk_batch* b, std::vector<Channel>& ch) {
    const size_t nb = ch.size();
    if (b->fmt.grind <= kGrindHostMaxBits || !b->grinder) {
        std::atomic<int> bad{0};
        b->pool->run(nb, 1, [&](size_t p) { uint64_t w; if (grind_channel(nullptr, ch[p], b->fmt.grind, &w)) bad.store(1); });
        return bad.load() ? fail(ZK_ERR_HIP, "zk_batch_prove: grinding failed") : (int)ZK_OK;
    }
    std::vector<uint8_t> states(32 * nb);
    std::vector<uint64_t> w(nb);
    for (size_t p = 0; p < nb; ++p) memcpy(states.data() + 32 * p, ch[p].state, 32);
    if (int rc = grind_device(b->grinder, states.data(), nb, b->fmt.grind, 0, w.data())) return rc;
    b->pool->run(nb, 16, [&](size_t p) { grind_commit(ch[p], w[p]); });
    return ZK_OK;
}
// the batch's roots of the last commit launch: [batch][8] state words in the mailbox
int bwait_roots(zk_batch* b) {
    const int rc = wait_flag(b->h_mail, b->mail_seq, b->stream);
    if (rc) b->counters_dirty = true;                     // see zk_ctx::counters_dirty (zkstark.hip)
    return rc;
}
// After bwait_roots: hashes the host's levels of every proof's tree `tree`, from its share h down to the depth ce the proofs commit
// (0: their roots), and returns where those digests are ([batch][2^ce][8] state words): the posted ones themselves when the device
// went all the way.
const uint32_t* bfinish_roots(zk_batch* b, uint32_t tree, uint32_t log_m, uint32_t lb) {
    const uint32_t ce = b->tree_cap[tree];
    const Hand hd = bhand(b, ce, log_m, lb);
    const uint32_t h = hd.h;
    const uint32_t* posted = (hd.mailbox ? b->h_mail : b->h_cap) + kMailDigests;
    if (!h) return posted;
    const size_t nb = (size_t)1 << lb;
    // stage[d], ce <= d < h: [proof][2^d] digests = level lb + d of the batch heap
    std::vector<uint32_t*> lvl(h + 1);
    for (uint32_t dd = ce; dd < h; ++dd) {
        lvl[dd] = b->h_stage + b->stage_used;
        b->stage_used += (nb << dd) * 8;
    }
    lvl[h] = const_cast<uint32_t*>(posted);
    b->pool->run(nb, 1, [&](size_t p) {
        for (uint32_t dd = h; dd-- > ce;) {
            const uint32_t* child = lvl[dd + 1] + ((p << (dd + 1)) * 8);
            uint32_t* out = lvl[dd] + ((p << dd) * 8);
            host_sha_inner_run(child, out, (size_t)1 << dd);
        }
    });
    for (uint32_t dd = ce; dd < h; ++dd) {
        b->h_segs[b->n_segs++] = ScatterSeg{(uint64_t)(lvl[dd] - b->h_stage),
                                            (uint64_t)b->tree_off[tree] + ((((uint64_t)1 << (lb + dd)) - 1) * 8),
                                            (uint32_t)((nb << dd) * 8), 0};
        b->seg_words += (double)((nb << dd) * 8);
    }
    return lvl[ce];
}

// values and path digests one query opens
void bopenings(const ProofFormat& f, size_t* vals, size_t* digs) {
    *vals = *digs = 0;
    f.for_each_tuple([&](size_t s, size_t plen, bool one_leaf, uint32_t words) { *vals += s * words; *digs += (one_leaf ? 1 : s) * plen; });
}
// gather buffers for q queries per proof (offsets in, values + digests out; device and pinned host copies), for the current fold
int balloc_gather(zk_batch* b, uint32_t q) {
    for (void* p : {(void*)b->d_goff, (void*)b->d_gout}) if (p) (void)hipFree(p);
    for (void* p : {(void*)b->h_goff, (void*)b->h_gout}) if (p) (void)hipHostFree(p);
    b->d_goff = nullptr; b->h_goff = nullptr; b->d_gout = nullptr; b->h_gout = nullptr;
    const size_t slots = b->batch * q * (b->per_proof_vals + b->per_proof_digs);
    const size_t out_words = b->batch * q * (b->per_proof_vals + 8 * b->per_proof_digs);
    HIPCHK(hipMalloc((void**)&b->d_goff, slots * 8));
    HIPCHK(hipMalloc((void**)&b->d_gout, out_words * 4));
    HIPCHK(hipHostMalloc((void**)&b->h_goff, slots * 8));
    HIPCHK(hipHostMalloc((void**)&b->h_gout, out_words * 4));
    b->fmt.q = q;
    return ZK_OK;
}

// The batch goes to the format `next` (fold, coset, stop, cap, ext; q and grind have setters of their own): d_work for the multi-fold (every
// fold > 1, and every fold with coset leaves or an early stop), the [batch][1 + 2^stop] tables of the final polynomials (two rows per proof
// with ext), the gather buffers for what a query of that format opens, the pinned buffer for caps the mailbox cannot hold and, when ext
// changes, d_layers with or without the planes, the component-1 challenge table and the constants of E.  Every new buffer is allocated
// before an old one goes: on failure the batch keeps its settings and the buffers they need.
int bset_format(zk_batch* b, const ProofFormat& next, const char* who) {
    const uint32_t stop = next.stop;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    if ((next.fold > 1 || next.coset || stop) && !b->d_work) {
        hipError_t e = hipMalloc((void**)&b->d_work, b->batch * 8 * 4);
        if (e != hipSuccess) return fail(ZK_ERR_NOMEM, "%s: hipMalloc(%zu) failed: %s", who, b->batch * 32, hipGetErrorString(e));
        b->device_bytes += b->batch * 32;
    }
    auto final_bytes = [&](const ProofFormat& f) { return f.stop ? (b->batch << f.ext) * (((size_t)1 << f.stop) + 1) * 4 : (size_t)0; };
    const bool ext_change = next.ext != b->fmt.ext, final_change = final_bytes(next) != final_bytes(b->fmt);
    uint32_t *nd_final = nullptr, *nh_final = nullptr;    // the new tables first: the old ones stay until nothing can fail any more
    uint32_t *nh_cap = nullptr, *nd_cap = nullptr, *nd_layers = nullptr, *nd_xwork = nullptr;
    BatchChalExt *nd_xchal = nullptr, *nh_xchal = nullptr;
    auto undo = [&] {
        for (void* p : {(void*)nd_final, (void*)nd_layers, (void*)nd_xwork, (void*)nd_xchal}) if (p) (void)hipFree(p);
        for (void* p : {(void*)nh_final, (void*)nh_cap, (void*)nh_xchal}) if (p) (void)hipHostFree(p);
    };
    if (final_change && stop) {
        hipError_t e = hipMalloc((void**)&nd_final, final_bytes(next));
        if (e == hipSuccess) e = hipHostMalloc((void**)&nh_final, final_bytes(next));
        if (e != hipSuccess) { undo(); return fail(ZK_ERR_NOMEM, "%s: allocating %zu bytes for the final polynomials failed: %s", who, final_bytes(next), hipGetErrorString(e)); }
    }
    const size_t cap_words = bcap_words(b, next);
    if (cap_words && cap_words != b->cap_words) {
        hipError_t e = hipHostMalloc((void**)&nh_cap, cap_words * 4, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&nd_cap, nh_cap, 0);
        if (e != hipSuccess) { undo(); return fail(ZK_ERR_NOMEM, "%s: allocating %zu pinned bytes for the Merkle caps failed: %s", who, cap_words * 4, hipGetErrorString(e)); }
    }
    // ext: the planes of the layers >= 1 behind the base layers; the component-1 challenges, plane 1 of the last layer, the constants of E
    const size_t plane_words = 2 * (b->layer_words - b->N * b->batch), xwork_bytes = b->batch * kFoldExtRow * 4, xchal_bytes = b->batch * sizeof(BatchChalExt);
    if (ext_change) {
        const size_t words = b->layer_words + (next.ext ? plane_words : 0);
        hipError_t e = hipMalloc((void**)&nd_layers, words * 4);
        if (e == hipSuccess && next.ext) e = hipMalloc((void**)&nd_xwork, xwork_bytes);
        if (e == hipSuccess && next.ext) e = hipMalloc((void**)&nd_xchal, xchal_bytes);
        if (e == hipSuccess && next.ext) e = hipHostMalloc((void**)&nh_xchal, xchal_bytes + b->batch * b->B * 4);
        if (e != hipSuccess) { undo(); return fail(ZK_ERR_NOMEM, "%s: allocating the layers of %zu words failed: %s", who, words, hipGetErrorString(e)); }
    }
    const size_t old_vals = b->per_proof_vals, old_digs = b->per_proof_digs;
    bopenings(next, &b->per_proof_vals, &b->per_proof_digs);
    if (int rc = balloc_gather(b, b->fmt.q)) {            // the old buffers are gone: put back what the old format needs, or fail again later
        b->per_proof_vals = old_vals; b->per_proof_digs = old_digs;
        (void)balloc_gather(b, b->fmt.q);
        undo();
        return rc;
    }
    if (cap_words != b->cap_words) {                      // cap 0, or a cap the mailbox holds, gives the buffer back
        if (b->h_cap) (void)hipHostFree(b->h_cap);
        b->device_bytes += cap_words * 4;
        b->device_bytes -= b->cap_words * 4;
        b->h_cap = nh_cap; b->d_cap = nd_cap; b->cap_words = cap_words;
    }
    if (final_change) {                                   // stop = 0 gives the tables back
        if (b->d_final) (void)hipFree(b->d_final);
        if (b->h_final) (void)hipHostFree(b->h_final);
        b->device_bytes += final_bytes(next);
        b->device_bytes -= final_bytes(b->fmt);
        b->d_final = nd_final; b->h_final = nh_final;
    }
    if (ext_change) {                                     // ext = 0 gives the planes and the tables of E back; the last proof's layers go
        for (void* p : {(void*)b->d_layers, (void*)b->d_xwork, (void*)b->d_xchal}) if (p) (void)hipFree(p);
        if (b->h_xchal) (void)hipHostFree(b->h_xchal);
        const size_t bytes = plane_words * 4 + xwork_bytes + xchal_bytes;
        if (next.ext) b->device_bytes += bytes; else b->device_bytes -= bytes;
        b->d_layers = nd_layers; b->d_xwork = nd_xwork; b->d_xchal = nd_xchal; b->h_xchal = nh_xchal;
        b->h_xlast = nh_xchal ? reinterpret_cast<uint32_t*>(nh_xchal + b->batch) : nullptr;
        b->ext_base = next.ext ? b->layer_words : 0;
    }
    b->fmt = next;
    return ZK_OK;
}

// the first `count` entries of the challenge table: the batch's for the alphas, afterwards one per channel
int bchal_upload(zk_batch* b, size_t count) {
    HIPCHK(hipMemcpyAsync(b->d_chal, b->h_chal, count * sizeof(BatchChal), hipMemcpyHostToDevice, b->stream));
    if (b->fmt.ext) HIPCHK(hipMemcpyAsync(b->d_xchal, b->h_xchal, count * sizeof(BatchChalExt), hipMemcpyHostToDevice, b->stream));   // component 1 beside
    return ZK_OK;
}

// ---- the pipeline.  One run of it makes the proofs of one call: as many as it has channels.
struct Run {
    zk_batch* b;
    ProofFormat f;                    // of the proofs made (zk_batch_prove: the batch's; shared: with lb and rows)
    std::vector<Channel> ch;          // 2^lb (zk_batch_prove), or one (zk_batch_prove_shared)
    uint32_t w;                       // width of the FRI stage, log2 of the trees built side by side from cp on: lb, or 0
    uint32_t fw;                      // ... and of the f stage: lb, or 0 with row leaves
    const char* who;                  // the entry point, for its errors
    double T0, t_wait = 0, t_caps = 0;   // ZK_HOST_TIMING: the last lap, waiting for the device, the pool hashing cap commits
    size_t nv = 0, ndg = 0;           // values and digests the queries of one channel open (run_queries)
};
bool btiming() { static const bool on = getenv("ZK_HOST_TIMING") != nullptr; return on; }
void lap(Run& r, const char* what) {
    if (!btiming()) return;
    double t = now_us();
    fprintf(stderr, "[zk batch timing] %-28s %8.1f us\n", what, t - r.T0);
    r.T0 = t;
}
int wait_roots(Run& r) { double t = now_us(); int rc = bwait_roots(r.b); r.t_wait += now_us() - t; return rc; }
// the pool's share of a commit round that hashes caps (ZK_HOST_TIMING)
void cap_lap(Run& r, uint32_t ce, double t) { if (btiming() && ce) r.t_caps += now_us() - t; }
// What a channel commits for a tree (prover.rs:85, :180, :224): the 2^ce digests of depth ce in ONE commit (ce = 0: the root).
// from: its [2^ce][8] state words (bfinish_roots).  A buffer on the stack: this runs once per proof and round on the pool.
void commit_cap(Channel& ch, const uint32_t* from, uint32_t ce) {
    uint8_t cb[32 << kMaxCapLog];
    for (size_t i = 0; i < ((size_t)1 << ce); ++i) digest_words_to_bytes(from + 8 * i, cb + 32 * i);
    ch.commit_bytes(cb, (size_t)32 << ce);
}
// The three alphas of statement p from `ch` (prover.rs:163-165) and its row of the challenge table.  g2 = g^2.
void balphas(zk_batch* b, size_t p, Channel& ch, uint32_t g2) {
    const uint32_t a0 = ch.get_u32() % P, a1 = ch.get_u32() % P, a2 = ch.get_u32() % P;
    BatchChal& c = b->h_chal[p];
    c.first = b->first[p]; c.last = b->last[p];
    c.alpha0_mont = to_mont(a0); c.alpha1g2_mont = to_mont(mulmod(a1, g2)); c.alpha2_mont = to_mont(a2);
}
// ... over E: six draws, alpha0.c0, alpha0.c1, alpha1.c0, .. (prove_ext_rounds' order); component 1 goes to the row of the table beside
void balphas_ext(zk_batch* b, size_t p, Channel& ch, uint32_t g2) {
    uint32_t a[6];
    for (uint32_t& v : a) v = ch.get_u32() % P;
    BatchChal& c = b->h_chal[p];
    c.first = b->first[p]; c.last = b->last[p];
    c.alpha0_mont = to_mont(a[0]); c.alpha1g2_mont = to_mont(mulmod(a[2], g2)); c.alpha2_mont = to_mont(a[4]);
    b->h_xchal[p] = BatchChalExt{to_mont(a[1]), to_mont(mulmod(a[3], g2)), to_mont(a[5]), 0u};
}
// The tree over layer `id` of a stage of width w: 2^log_len values per proof, 2^leaf_steps to a leaf (0: one-value leaves, prover.rs:214).
// ext: the layer is two planes and a leaf hashes its component-0 words, then its component-1 words (transcript.hpp "ext").  With one-value
// leaves the batch heap over 2^(w + log_len) leaves IS the row tree of the [2][2^(w + log_len)] array the planes are; with coset leaves the
// slots of a leaf are strided inside one proof and the leaves come from a launch of their own.  Same heap, same hand-over either way.
int btree(zk_batch* b, uint32_t id, uint32_t log_len, uint32_t leaf_steps, uint32_t w, bool ext = false) {
    b->tree_steps[id] = (uint8_t)leaf_steps;
    if (ext && leaf_steps) HIPCHK(launch_merkle_build_coset_ext_batch(bext_layer(b, id), log_len, leaf_steps, w, b->d_trees + b->tree_off[id], b->stream, nullptr,
                                                                      bmail(b, id, log_len - leaf_steps, w), b->hash));
    else if (ext) HIPCHK(launch_merkle_build_rows(bext_layer(b, id), log_len + w, 1, b->d_trees + b->tree_off[id], b->stream, nullptr, bmail(b, id, log_len, w), b->hash));
    else if (leaf_steps) HIPCHK(launch_merkle_build_coset_batch(b->d_layers + b->layer_off[id], log_len, leaf_steps, w, b->d_trees + b->tree_off[id], b->stream, nullptr,
                                                           bmail(b, id, log_len - leaf_steps, w), b->hash));
    else HIPCHK(launch_merkle_build(b->d_layers + b->layer_off[id], log_len + w, b->d_trees + b->tree_off[id], b->stream, nullptr, bmail(b, id, log_len, w), b->hash));
    return bpost(b, id, log_len - leaf_steps, w);
}

// f = the LDE of every trace (prover.rs:60-85) and its tree at width fw -- the batch heap, or the one tree over the rows -- with the
// bookkeeping of a new proof (skipped: the trees it will not have built for the batch, to which run_groups adds).  Returns with tree 0
// handed over and finished (*roots: 2^(fw + ce) digests) and the proof-independent part of cp's constants (compose_args with alpha = 1).
int run_commit_f(Run& r, uint64_t skipped, ComposeBatchArgs& ca, const uint32_t** roots) {
    zk_batch* b = r.b;
    const uint32_t L = b->L, lb = b->lb;
    uint32_t* f0 = b->d_layers + b->layer_off[0];
    int rc;
    if ((rc = dom_lde(b->dom, b->d_trace, b->d_coef, f0, b->stream, nullptr, (uint32_t)b->batch))) return rc;
    b->stage_used = 0; b->n_segs = 0; b->seg_words = 0;
    b->skipped_trees = skipped; b->proved_fold = r.f.fold; b->proved_stop = r.f.stop; b->proved_hash = b->hash;
    memset(b->tree_steps, 0, sizeof b->tree_steps);
    memset(b->tree_cap, 0, sizeof b->tree_cap);
    b->proved = true; b->rows_tree0 = r.f.rows;
    if (r.f.rows) HIPCHK(launch_merkle_build_rows(f0, L, lb, b->d_trees + b->tree_off[0], b->stream, nullptr, bmail(b, 0, L, 0), b->hash));
    else HIPCHK(launch_merkle_build(f0, L + lb, b->d_trees + b->tree_off[0], b->stream, nullptr, bmail(b, 0, L, lb), b->hash));
    if ((rc = bpost(b, 0, L, r.fw))) return rc;
    const uint32_t one[3] = {1, 1, 1};
    if ((rc = compose_args(b->dom, f0, b->d_layers + b->layer_off[1], 0, 0, one, ca.a))) return rc;
    ca.chal = b->d_chal;
    if ((rc = wait_roots(r))) return rc;
    *roots = bfinish_roots(b, 0, L, r.fw);
    return ZK_OK;
}

// The groups of `fold` rounds, from "tree 1 is built and posted" to "the last tree is committed" or, with an early stop, "the layer
// the proofs stop at is folded" (it gets no tree, no wait and no root).  Per group: the roots arrive, every channel commits its tree and
// draws its beta (prover.rs:180 / :224, :200) into its row of the table, the rows go up, and the fold and the next tree are launched --
// one fused launch when K = 1 without coset leaves or stop (prover.rs:201-214), else the multi-fold (prover.rs:201-211, steps times)
// and a tree over the next group's input, whose leaves are that group's cosets (the last layer: one value).
int run_groups(Run& r) {
    zk_batch* b = r.b;
    const ProofFormat& f = r.f;
    const zk_dom* d = b->dom;
    const size_t np = r.ch.size();
    const uint32_t w = r.w, L = b->L, G = f.groups();
    const bool fused = f.fold == 1 && !f.coset && !f.stop && !f.ext;      // the fold inside the leaf hashing of its tree
    int rc;
    for (uint32_t j = 0;; ++j) {                                          // tree 1 + r0 is the last one launched
        const uint32_t r0 = f.round0(j);
        if ((rc = wait_roots(r))) return rc;
        const uint32_t* roots = bfinish_roots(b, 1 + r0, L - r0 - b->tree_steps[1 + r0], w);   // 2^(L - r0) values per proof, 2^tree_steps per leaf
        const uint32_t ce = b->tree_cap[1 + r0];                          // ... committed by its 2^ce digests of depth ce
        const double tc = btiming() ? now_us() : 0;
        if (j == G) {
            b->pool->run(np, 32, [&](size_t p) { commit_cap(r.ch[p], roots + ((p << ce) * 8), ce); });
            cap_lap(r, ce, tc);
            break;
        }
        const uint32_t steps = f.steps(j), id = f.tree_id(j + 1);
        // K = 1: the fold constant is reduced on the host; otherwise the challenge goes up RAW and is reduced on the device
        const uint32_t winv_half = fused ? mulmod(invmod(powmod(d->shift, (uint64_t)1 << r0)), invmod(2)) : 0;
        b->pool->run(np, 32, [&](size_t p) {
            commit_cap(r.ch[p], roots + ((p << ce) * 8), ce);
            const uint32_t beta = r.ch[p].get_u32();
            b->h_chal[p].c_mont = fused ? to_mont(mulmod(beta % P, winv_half)) : beta;
            if (f.ext) b->h_xchal[p].beta1 = r.ch[p].get_u32();           // beta.c1, raw as well (prove_ext_rounds)
        });
        cap_lap(r, ce, tc);
        if ((rc = bchal_upload(b, np))) return rc;
        if (fused) {
            FoldBatchArgs fa;
            if ((rc = fold_args(d, b->d_layers + b->layer_off[1 + r0], b->d_layers + b->layer_off[id], L - r0, r0, 0, fa.a))) return rc;
            fa.chal = b->d_chal;
            HIPCHK(launch_fold_merkle_batch(fa, w, b->d_trees + b->tree_off[id], b->stream, nullptr, bmail(b, id, L - r0 - 1, w), b->hash));
            if ((rc = bpost(b, id, L - r0 - 1, w))) return rc;
            continue;
        }
        if (f.ext) {                                                      // the same butterfly over E, both planes in one launch
            if ((rc = dom_fold_multi_ext_batch(d, bext_layer(b, 1 + r0), bext_layer(b, id), L - r0, r0, steps, &b->d_chal->c_mont, (uint32_t)(sizeof(BatchChal) / 4),
                                               &b->d_xchal->beta1, (uint32_t)(sizeof(BatchChalExt) / 4), b->d_xwork, (uint32_t)np, b->stream, nullptr))) return rc;
        } else if ((rc = dom_fold_multi_batch(d, b->d_layers + b->layer_off[1 + r0], b->d_layers + b->layer_off[id], L - r0, r0, steps, &b->d_chal->c_mont,
                                              (uint32_t)(sizeof(BatchChal) / 4), b->d_work, (uint32_t)np, b->stream, nullptr))) return rc;
        for (uint32_t l = 2 + r0; l < id; ++l) b->skipped_trees |= (uint64_t)1 << l;
        if (f.stop && j + 1 == G) {
            for (uint32_t l = id; l <= b->R + 1; ++l) b->skipped_trees |= (uint64_t)1 << l;
            break;
        }
        if ((rc = btree(b, id, L - r0 - steps, f.slots_log(j + 1), w, f.ext != 0))) return rc;
    }
    lap(r, "lde .. last roots");
    if (btiming()) fprintf(stderr, "[zk batch timing]   of which waiting for the device %.1f us\n", r.t_wait);
    if (btiming() && f.cap) fprintf(stderr, "[zk batch timing]   of which host threads hashing cap commits %.1f us\n", r.t_caps);
    return ZK_OK;
}

// The end of FRI.  Early stop: one launch turns layer 1 + R' (2^(stop + log_b) values per proof) into the rows (count, c_0 .. c_(2^stop - 1))
// of h_final, and every coefficient of degree >= 2^stop must be zero; else the last layer is B equal values per proof (prover.rs:238, :251).
// Each channel then commits its free term (prover.rs:254) or its 4 * 2^stop coefficient bytes in one commit (transcript.hpp "stop"),
// grinds, and draws its Q query raws (prover.rs:263); the offsets of what they open go to h_goff: channel c's value words at c * nv,
// its digests at np * nv + c * ndg.
int run_queries(Run& r) {
    zk_batch* b = r.b;
    const ProofFormat& f = r.f;
    const size_t np = r.ch.size(), N = b->N, B = b->B;
    const uint32_t stop = f.stop, Rp = f.rounds(), L = b->L, Q = f.q;
    const size_t ncoef = (size_t)1 << stop, frow = ncoef + 1;
    static const char kWhich[] = "some trace of the batch does not satisfy the constraints (the sum does not tell which)";
    const bool shared = f.lb != 0;                                        // whose failure no single trace answers for
    const size_t planes = (size_t)1 << f.ext;                             // ext: plane 1's layers, rows and values follow plane 0's np
    int rc;
    if (stop) {
        const uint32_t* last = f.ext ? bext_layer(b, 1 + Rp) : b->d_layers + b->layer_off[1 + Rp];
        if ((rc = dom_final_poly_batch(b->dom, last, b->d_final, L - Rp, Rp, (uint32_t)ncoef, (uint32_t)(planes * np), b->stream, nullptr))) return rc;
        HIPCHK(hipMemcpyAsync(b->h_final, b->d_final, planes * np * frow * 4, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        for (size_t p = 0; p < np; ++p) {
            const uint32_t above = b->h_final[p * frow] + (f.ext ? b->h_final[(np + p) * frow] : 0u);   // either plane's high coefficients
            if (above && shared) return fail(ZK_ERR_CHECK, "%s: final FRI layer has degree >= 2^%u (%u non-zero coefficients above): %s", r.who, stop, above, kWhich);
            if (above)
                return fail(ZK_ERR_CHECK, "proof %zu of the batch: final FRI layer has degree >= 2^%u: its trace does not satisfy the constraints (%u non-zero coefficients above; cf. prover.rs:238)",
                            p, stop, above);
        }
    } else {
        const uint32_t* last = f.ext ? bext_layer(b, 1 + b->R) : b->d_layers + b->layer_off[1 + b->R];
        HIPCHK(hipMemcpyAsync(b->h_last, last, np * B * 4, hipMemcpyDeviceToHost, b->stream));
        if (f.ext) HIPCHK(hipMemcpyAsync(b->h_xlast, last + np * B, np * B * 4, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        for (size_t p = 0; p < np; ++p)
            for (size_t i = 1; i < B; ++i) {
                if (b->h_last[p * B + i] == b->h_last[p * B] && (!f.ext || b->h_xlast[p * B + i] == b->h_xlast[p * B])) continue;
                if (shared) return fail(ZK_ERR_CHECK, "%s: last FRI layer is not constant (prover.rs:238): %s", r.who, kWhich);
                return fail(ZK_ERR_CHECK, "proof %zu of the batch: last FRI layer is not constant (prover.rs:238): its trace does not satisfy the constraints", p);
            }
    }
    // ext: (c0, c1) of the free term, or the 2^stop component-0 coefficients, then the component-1 ones, in ONE commit (prove_finish)
    auto commit_final = [&](size_t p) {
        if (!stop && !f.ext) { r.ch[p].commit_u32(b->h_last[p * B]); return; }
        uint8_t cb[8 << kMaxStopLog];
        size_t n = 0;
        auto put = [&](uint32_t v) { for (int i = 0; i < 4; ++i) cb[n++] = (uint8_t)(v >> (8 * i)); };
        for (size_t plane = 0; plane < planes; ++plane) {
            if (!stop) { put(plane ? b->h_xlast[p * B] : b->h_last[p * B]); continue; }
            const uint32_t* c = b->h_final + (plane * np + p) * frow + 1;
            for (size_t k = 0; k < ncoef; ++k) put(c[k]);
        }
        r.ch[p].commit_bytes(cb, n);
    };
    bopenings(f, &r.nv, &r.ndg);
    r.nv *= Q; r.ndg *= Q;
    const size_t nv = r.nv, ndg = r.ndg;
    if (f.grind) {                                                        // free terms, then the nonces of all channels at once
        b->pool->run(np, 16, [&](size_t p) { commit_final(p); });
        if ((rc = bgrind(b, r.ch))) return rc;
        lap(r, "grind");
    }
    std::atomic<int> bad{0};
    b->pool->run(np, 16, [&](size_t c) {
        if (!f.grind) commit_final(c);
        uint32_t qraw[kMaxQueries];
        for (uint32_t k = 0; k < Q; ++k) qraw[k] = r.ch[c].get_u32();     // prover.rs:263 (x Q)
        uint64_t *const vo0 = b->h_goff + c * nv, *const do0 = b->h_goff + np * nv + c * ndg;
        uint64_t *vo = vo0, *dofs = do0;
        std::vector<size_t> nodes;
        // An opening (prover.rs:263-289) is a leaf of `layer` in a stage of width wl = fw (layer 0) or w, of the proof p of that stage:
        // this channel's (the walk has lb = 0: the leaf is its index in the proof's layer), or, for the f leaves of a shared proof without
        // rows, the statement the leaf index leads with (at every other layer it leads with 0).  One of the two terms of p is zero.
        // Layer l is stored proof-major, so the 2^slots_log values of the leaf (one unless coset or row leaves) are words
        // (p << (log_m + slots_log)) + at + (u << log_m) of it; node (depth dd, index i) of the proof's tree over 2^log_m leaves is node
        // 2^(wl + dd) - 1 + p 2^dd + i of the heap; path_nodes walks from the leaf level up, and the path ends below the tree's cap.
        for (uint32_t k = 0; k < Q; ++k)
            f.for_each_opening((size_t)qraw[k] % (N - 2 * B), [&](uint32_t layer, uint32_t log_m, size_t leaf, uint32_t slots_log) {
                const uint32_t wl = layer == 0 ? r.fw : r.w;
                const size_t p = c + (leaf >> log_m), at = leaf & (((size_t)1 << log_m) - 1);
                if (f.ext && layer >= 1) {                                // a leaf of E: its component-0 slots, then its component-1 slots
                    for (size_t plane = 0; plane < 2; ++plane)
                        for (size_t u = 0; u < ((size_t)1 << slots_log); ++u)
                            *vo++ = bext_off(b, layer) + ((plane * np + p) << (log_m + slots_log)) + at + (u << log_m);
                } else for (size_t u = 0; u < ((size_t)1 << slots_log); ++u) *vo++ = b->layer_off[layer] + (p << (log_m + slots_log)) + at + (u << log_m);
                nodes.clear();
                path_nodes((size_t)1 << log_m, at, nodes);
                nodes.resize(log_m - b->tree_cap[layer]);
                uint32_t dd = log_m;
                for (size_t nd : nodes) {
                    const size_t i = nd - (((size_t)1 << dd) - 1);
                    *dofs++ = (uint64_t)b->tree_off[layer] + (uint64_t)((((size_t)1 << (wl + dd)) - 1) + (p << dd) + i) * 8;
                    --dd;
                }
            });
        if ((size_t)(vo - vo0) != nv || (size_t)(dofs - do0) != ndg) bad.store(1);
    });
    lap(r, "queries + opening offsets");
    return bad.load() ? fail(ZK_ERR_STATE, "%s: unexpected number of openings", r.who) : (int)ZK_OK;
}

// The openings themselves: the host-built levels go into the trees, two gathers fetch every channel's values and digests, and each channel
// commits its tuples (prover.rs:274-277, then per group prover.rs:280-289).  Channel c's proof goes to proofs_out + c * stride, its
// Channel.state to states_out + 32 c (channel.rs:34-36).
int run_decommit(Run& r, uint8_t* proofs_out, size_t stride, uint8_t* states_out) {
    zk_batch* b = r.b;
    const ProofFormat& f = r.f;
    const size_t np = r.ch.size(), nv = r.nv, ndg = r.ndg, tv = np * nv, td = np * ndg, plen = f.data_len();
    HIPCHK(hipMemcpyAsync(b->d_goff, b->h_goff, (tv + td) * 8, hipMemcpyHostToDevice, b->stream));
    HIPCHK(launch_scatter(b->d_stage, b->d_segs, b->n_segs, b->seg_words, b->d_trees, nullptr, b->stream, nullptr));   // host-built levels
    HIPCHK(launch_gather(b->d_layers, b->d_goff, (uint32_t)tv, 1, b->d_gout, b->stream, nullptr));
    HIPCHK(launch_gather(b->d_trees, b->d_goff + tv, (uint32_t)td, 8, b->d_gout + tv, b->stream, nullptr));
    HIPCHK(hipMemcpyAsync(b->h_gout, b->d_gout, (tv + td * 8) * 4, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    lap(r, "gather");
    size_t widest = ProofFormat::tuple_bytes((size_t)1 << f.steps(0), b->L, false, 1u << f.ext);   // the first group's tuple, or a row of 2^lb values
    if (f.rows && Channel::group_bytes(b->batch, b->L, true) > widest) widest = Channel::group_bytes(b->batch, b->L, true);
    std::atomic<int> bad{0};
    b->pool->run(np, 4, [&](size_t c) {
        Channel& ch = r.ch[c];
        const uint32_t* vals = b->h_gout + c * nv;
        const uint32_t* dw = b->h_gout + tv + c * ndg * 8;
        std::vector<uint8_t> buf(widest);                                 // one buffer per channel
        // the values were gathered opening by opening (for a value of E: c0, c1); a tuple of s openings sends the s c0 words, then the s c1 words
        auto tuple = [&](size_t s, size_t pl, bool one_leaf, uint32_t words) {
            ch.commit_group(buf.data(), s, pl, [&](size_t t) { return vals[words == 2 && !one_leaf ? (t % s) * 2 + t / s : t]; },
                            [&](size_t i, uint8_t* out) { digest_words_to_bytes(dw + 8 * i, out); }, one_leaf, words);
            vals += s * words; dw += 8 * (one_leaf ? 1 : s) * pl;
        };
        for (uint32_t q = 0; q < f.q; ++q) f.for_each_tuple(tuple);
        if (ch.data.size() != plen) { bad.store(1); return; }
        memcpy(proofs_out + c * stride, ch.data.data(), plen);
        memcpy(states_out + 32 * c, ch.state, 32);
    });
    lap(r, "decommit hashing + copy out");
    return bad.load() ? fail(ZK_ERR_STATE, "%s: unexpected proof length", r.who) : (int)ZK_OK;
}

}  // namespace

extern "C" {

int zk_batch_destroy(zk_batch* b) {
    if (!b) return ZK_OK;
    (void)hipSetDevice(b->device);
    if (b->single) zk_ctx_destroy(b->single);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    dom_free(b->dom);
    for (void* p : {(void*)b->d_trace, (void*)b->d_coef, (void*)b->d_layers, (void*)b->d_trees, (void*)b->d_seed, (void*)b->d_chal,
                    (void*)b->d_counter, (void*)b->d_goff, (void*)b->d_gout, (void*)b->d_work, (void*)b->d_final, (void*)b->d_xwork, (void*)b->d_xchal})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)b->h_chal, (void*)b->h_mail, (void*)b->h_goff, (void*)b->h_gout, (void*)b->h_last, (void*)b->h_stage, (void*)b->h_final, (void*)b->h_cap, (void*)b->h_xchal})
        if (p) (void)hipHostFree(p);
    grinder_destroy(b->grinder);                         // on b->stream: before the stream goes
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b->pool;
    delete b;
    return ZK_OK;
}

int zk_batch_create(int device, uint32_t log_n, uint32_t log_b, uint32_t log_batch, zk_batch** out) {
    if (!out) return fail(ZK_ERR_INVALID, "zk_batch_create: out is null");
    *out = nullptr;
    if (log_batch > kMaxHostLog) return fail(ZK_ERR_INVALID, "zk_batch_create: need log_batch <= %u", kMaxHostLog);
    if (int rc0 = check_proof_size("zk_batch_create", log_n, log_b, log_batch)) return rc0;   // the same sizes zk_ctx_create accepts
    HIPCHK(hipSetDevice(device));
    zk_batch* b = new (std::nothrow) zk_batch();
    if (!b) return fail(ZK_ERR_NOMEM, "out of host memory");
    b->device = device;
    b->fmt.log_n = log_n; b->fmt.log_b = log_b;
    b->log_n = log_n; b->log_b = log_b; b->lb = log_batch; b->L = log_n + log_b; b->R = log_n;
    b->n = (size_t)1 << log_n; b->B = (size_t)1 << log_b; b->N = b->n << log_b; b->batch = (size_t)1 << log_batch;
    int rc = ZK_OK;
    auto bail = [&](int code) { zk_batch_destroy(b); return code; };
    if (log_batch == 0) {                                  // one proof: the single prover
        if ((rc = zk_ctx_create(device, log_n, log_b, &b->single))) return bail(rc);
        b->first.assign(1, 0);
        b->last.assign(1, 0);
        b->device_bytes = zk_ctx_device_bytes(b->single);
        *out = b;
        return ZK_OK;
    }
#define HIPCHK_B(expr)                                                                        \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            zk_batch_destroy(b);                                                              \
            return fail(ZK_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                     \
    } while (0)
    HIPCHK_B(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    if ((rc = dom_make(device, log_n, log_b, GEN_W, false, b->stream, &b->dom))) return bail(rc);
    b->device_bytes += b->dom->device_bytes;
    size_t off = 0;
    for (uint32_t l = 0; l <= b->R + 1; ++l) { b->layer_off.push_back(off); off += blayer_size(b, l) * b->batch; }
    const size_t layer_words = off;
    b->layer_words = layer_words;
    off = 0;
    for (uint32_t l = 0; l <= b->R + 1; ++l) { b->tree_off.push_back(off); off += (2 * blayer_size(b, l) * b->batch - 1) * 8; }
    const size_t tree_words = off;
    auto dm = [&](auto** p, size_t bytes) {
        hipError_t e = hipMalloc((void**)p, bytes ? bytes : 4);
        if (e != hipSuccess) return fail(ZK_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        b->device_bytes += bytes;
        return (int)ZK_OK;
    };
    if ((rc = dm(&b->d_trace, b->batch * b->n * 4)) || (rc = dm(&b->d_coef, b->batch * 2 * b->n * 4)) ||
        (rc = dm(&b->d_layers, layer_words * 4)) || (rc = dm(&b->d_trees, tree_words * 4)) || (rc = dm(&b->d_seed, 2 * b->batch * 4)) ||
        (rc = dm(&b->d_chal, b->batch * sizeof(BatchChal))) || (rc = dm(&b->d_counter, 64)))
        return bail(rc);
    HIPCHK_B(hipMemsetAsync(b->d_counter, 0, 64, b->stream));
    HIPCHK_B(hipMemsetAsync(b->d_trace, 0, b->batch * b->n * 4, b->stream));
    bopenings(b->fmt, &b->per_proof_vals, &b->per_proof_digs);
    if ((rc = balloc_gather(b, 1))) return bail(rc);
    HIPCHK_B(hipHostMalloc((void**)&b->h_chal, b->batch * sizeof(BatchChal)));
    HIPCHK_B(hipHostMalloc((void**)&b->h_last, b->batch * (b->B > 2 ? b->B : 2) * 4));
    HIPCHK_B(hipHostMalloc((void**)&b->h_mail, kMailWords * 4, hipHostMallocMapped | hipHostMallocCoherent));
    memset(b->h_mail, 0, kMailWords * 4);
    memset(b->h_chal, 0, b->batch * sizeof(BatchChal));
    HIPCHK_B(hipHostGetDevicePointer((void**)&b->d_mail, b->h_mail, 0));
    b->stage_words = (size_t)(b->R + 2) * ((size_t)8 << kMaxHostLog);
    const size_t seg_bytes = (size_t)(b->R + 2) * kMaxHostLog * sizeof(ScatterSeg);
    HIPCHK_B(hipHostMalloc((void**)&b->h_stage, b->stage_words * 4 + seg_bytes, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK_B(hipHostGetDevicePointer((void**)&b->d_stage, b->h_stage, 0));
    b->h_segs = reinterpret_cast<ScatterSeg*>(b->h_stage + b->stage_words);
    b->d_segs = reinterpret_cast<ScatterSeg*>(b->d_stage + b->stage_words);
    b->host_levels = host_sha_available();               // zk_batch_set_host_levels(b, 0) keeps every level on the device
    HIPCHK_B(hipStreamSynchronize(b->stream));
#undef HIPCHK_B
    b->first.assign(b->batch, 0);
    b->last.assign(b->batch, 0);
    unsigned hw = std::thread::hardware_concurrency();
    unsigned want = hw > 1 ? (hw - 1 < 15 ? hw - 1 : 15) : 0;
    if (b->batch < 2) want = 0;
    b->pool = new (std::nothrow) Pool(want);
    if (!b->pool) return bail(fail(ZK_ERR_NOMEM, "out of host memory"));
    *out = b;
    return ZK_OK;
}

size_t zk_batch_size(const zk_batch* b) { return b ? b->batch : 0; }
// One batch is used from one host thread at a time (include/zkstark_amd.h); a setter that arrives while zk_batch_prove runs on
// another thread would pull the pool, the gather buffers or the traces from under it, so it is refused instead.
struct BusyScope {
    zk_batch* b; bool mine;
    explicit BusyScope(zk_batch* b_) : b(b_) { bool expected = false; mine = b->busy.compare_exchange_strong(expected, true, std::memory_order_acq_rel); }
    ~BusyScope() { if (mine) b->busy.store(false, std::memory_order_release); }
};
// (the setters hold the same flag for their own duration, so a prove that starts while a setter replaces the pool is refused too)
#define ZK_BATCH_EXCLUSIVE(b, who)                                                                       \
    BusyScope _excl(b);                                                                                  \
    if (!_excl.mine) return fail(ZK_ERR_STATE, "%s: another call (zk_batch_prove or a setter) is running on this batch", who)
int zk_batch_set_host_levels(zk_batch* b, int on) {
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_host_levels");
    if (b->single) return zk_ctx_set_host_levels(b->single, on && host_sha_available() ? 8 : 0, on && host_sha_available() ? 9 : 0);
    b->host_levels = on != 0 && host_sha_available();
    return ZK_OK;
}
int zk_batch_set_threads(zk_batch* b, uint32_t threads) {
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_threads");
    if (threads < 1 || threads > 64) return fail(ZK_ERR_INVALID, "zk_batch_set_threads: need 1 <= threads <= 64");
    if (b->single || !b->pool || b->pool->workers() == threads - 1) return ZK_OK;
    Pool* np = new (std::nothrow) Pool(threads - 1);
    if (!np) return fail(ZK_ERR_NOMEM, "out of host memory");
    delete b->pool;
    b->pool = np;
    return ZK_OK;
}
int zk_batch_set_queries(zk_batch* b, uint32_t n_queries) {
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_queries");
    if (n_queries < 1 || n_queries > 16) return fail(ZK_ERR_INVALID, "zk_batch_set_queries: need 1 <= n_queries <= 16");
    if (b->single) { b->fmt.q = n_queries; return zk_ctx_set_queries(b->single, n_queries); }
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    return n_queries == b->fmt.q ? (int)ZK_OK : balloc_gather(b, n_queries);
}
int zk_batch_set_hash(zk_batch* b, int hash_kind) {
    // refused before the handle is looked at: no setting of this class takes it
    if (hash_kind == ZK_HASH_BLAKE2S) return fail(ZK_ERR_INVALID, "zk_batch_set_hash: BLAKE2s (hash 2) is not built for this entry point yet");
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_hash");
    if (hash_kind != ZK_HASH_SHA256 && hash_kind != ZK_HASH_FIELD) return fail(ZK_ERR_INVALID, "zk_batch_set_hash: unknown hash %d", hash_kind);
    b->hash = hash_kind;
    if (b->single) return zk_ctx_set_hash(b->single, hash_kind);
    return ZK_OK;
}
int zk_batch_set_grinding(zk_batch* b, uint32_t grind_bits) {
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_grinding");
    if (grind_bits > kMaxGrindBits) return fail(ZK_ERR_INVALID, "zk_batch_set_grinding: need grind_bits <= %u (got %u)", kMaxGrindBits, grind_bits);
    if (b->single) { b->fmt.grind = grind_bits; return zk_ctx_set_grinding(b->single, grind_bits); }
    if (grind_bits > kGrindHostMaxBits && !b->grinder) {
        HIPCHK(hipSetDevice(b->device));
        if (int rc = grinder_create(b->device, b->stream, (uint32_t)b->batch, &b->grinder)) return rc;
    }
    b->fmt.grind = grind_bits;
    return ZK_OK;
}
// FRI folding factor 2^fold_log between commitments (include/zkstark_amd.h).  A query of a folded proof opens 2^steps values and paths
// per group: the gather buffers are re-sized here, as zk_ctx_set_fold does, not inside the first proof.
int zk_batch_set_fold(zk_batch* b, uint32_t fold_log) {
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_fold");
    if (fold_log < 1 || fold_log > kMaxFoldLog) return fail(ZK_ERR_INVALID, "zk_batch_set_fold: need 1 <= fold_log <= %u (got %u)", kMaxFoldLog, fold_log);
    if (b->single) {
        if (int rc = zk_ctx_set_fold(b->single, fold_log)) return rc;
        b->fmt.fold = fold_log;
        return ZK_OK;
    }
    if (fold_log == b->fmt.fold) return ZK_OK;
    ProofFormat next = b->fmt;
    next.fold = fold_log;
    return bset_format(b, next, "zk_batch_set_fold");
}
uint32_t zk_batch_get_fold(const zk_batch* b) { return b ? b->fmt.fold : 0; }
// Coset leaves (include/zkstark_amd.h): from the next zk_batch_prove on.  A coset proof opens fewer nodes and other values than a plain
// one, so the gather buffers are re-sized here; every fold, 1 included, then runs on the multi-fold and needs d_work.
int zk_batch_set_coset_leaves(zk_batch* b, int on) {
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_coset_leaves");
    if (b->single) {
        if (int rc = zk_ctx_set_coset_leaves(b->single, on)) return rc;
        b->fmt.coset = on != 0;
        return ZK_OK;
    }
    if ((on != 0) == b->fmt.coset) return ZK_OK;
    ProofFormat next = b->fmt;
    next.coset = on != 0;
    return bset_format(b, next, "zk_batch_set_coset_leaves");
}
int zk_batch_get_coset_leaves(const zk_batch* b) { return b && b->fmt.coset ? 1 : 0; }
// Early stop (include/zkstark_amd.h): from the next zk_batch_prove on.  A stopped proof opens only the groups of log_n - stop_log rounds,
// so the gather buffers are re-sized here; every fold, 1 included, then runs on the multi-fold and needs d_work, and the tables of the
// final polynomials are allocated for this stop_log.
int zk_batch_set_fri_stop(zk_batch* b, uint32_t stop_log) {
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_fri_stop");
    if (!stop_ok(b->log_n, b->log_b, stop_log))
        return fail(ZK_ERR_INVALID, "zk_batch_set_fri_stop: need stop_log <= %u, stop_log <= log_n - 1 = %u and stop_log + log_blowup <= %u (got %u)",
                    kMaxStopLog, b->log_n - 1, kMaxStopLayerLog, stop_log);
    if (b->single) {
        if (int rc = zk_ctx_set_fri_stop(b->single, stop_log)) return rc;
        b->fmt.stop = stop_log;
        return ZK_OK;
    }
    if (stop_log == b->fmt.stop) return ZK_OK;
    ProofFormat next = b->fmt;
    next.stop = stop_log;
    return bset_format(b, next, "zk_batch_set_fri_stop");
}
uint32_t zk_batch_get_fri_stop(const zk_batch* b) { return b ? b->fmt.stop : 0; }
// Merkle caps (include/zkstark_amd.h): from the next zk_batch_prove on.  A capped proof opens shorter paths, so the gather buffers are
// re-sized here; a cap that lies deeper in the batch heap than the mailbox holds gets its pinned buffer here, not inside the first proof.
int zk_batch_set_merkle_cap(zk_batch* b, uint32_t cap_log) {
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_merkle_cap");
    if (cap_log > kMaxCapLog) return fail(ZK_ERR_INVALID, "zk_batch_set_merkle_cap: need cap_log <= %u (got %u)", kMaxCapLog, cap_log);
    if (b->single) {
        if (int rc = zk_ctx_set_merkle_cap(b->single, cap_log)) return rc;
        b->fmt.cap = cap_log;
        return ZK_OK;
    }
    if (cap_log == b->fmt.cap) return ZK_OK;
    ProofFormat next = b->fmt;
    next.cap = cap_log;
    return bset_format(b, next, "zk_batch_set_merkle_cap");
}
uint32_t zk_batch_get_merkle_cap(const zk_batch* b) { return b ? b->fmt.cap : 0; }
// Challenges in E (include/zkstark_amd.h): from the next zk_batch_prove on.  An ext proof opens two words per value of cp and
// of the FRI layers, its layers >= 1 are two planes each and its final polynomial has two rows, so everything is sized here, both ways:
// with ext off every allocation is what it was.
int zk_batch_set_ext(zk_batch* b, uint32_t ext_log) {
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    if (ext_log > 1) return fail(ZK_ERR_INVALID, "zk_batch_set_ext: ext_log must be 0 or 1 (got %u; 2, the quartic extension, is reserved)", ext_log);
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_ext");
    if (b->single) {
        if (int rc = zk_ctx_set_ext(b->single, ext_log)) return rc;
        b->fmt.ext = ext_log;
        b->device_bytes = zk_ctx_device_bytes(b->single);
        return ZK_OK;
    }
    if (ext_log == b->fmt.ext) return ZK_OK;
    ProofFormat next = b->fmt;
    next.ext = ext_log;
    return bset_format(b, next, "zk_batch_set_ext");
}
uint32_t zk_batch_get_ext(const zk_batch* b) { return b ? b->fmt.ext : 0; }
// Row leaves (include/zkstark_amd.h): from the next zk_batch_prove_shared on; zk_batch_prove does not look at it.  A query of such a proof
// opens as many values and fewer digests than one of a shared proof without, so the gather buffers stay as they are.
int zk_batch_set_shared_rows(zk_batch* b, int on) {
    if (!b) return fail(ZK_ERR_INVALID, "null batch");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_shared_rows");
    b->shared_rows = on != 0;
    return ZK_OK;
}
int zk_batch_get_shared_rows(const zk_batch* b) { return b && b->shared_rows ? 1 : 0; }
uint32_t zk_batch_merkle_cap_log(const zk_batch* b, uint32_t tree) {
    if (!b) return 0;
    if (b->single) return zk_ctx_merkle_cap_log(b->single, tree);
    return tree <= b->R + 1 ? b->tree_cap[tree] : 0;
}
size_t zk_batch_device_bytes(const zk_batch* b) { return b ? b->device_bytes : 0; }

// traces: [batch][n-1] canonical residues on the host (prover.rs:32-39 per proof)
static int set_traces_exclusive(zk_batch* b, const uint32_t* traces);
int zk_batch_set_traces(zk_batch* b, const uint32_t* traces) {
    if (!b || !traces) return fail(ZK_ERR_INVALID, "zk_batch_set_traces: null argument");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_set_traces");
    return set_traces_exclusive(b, traces);
}
static int set_traces_exclusive(zk_batch* b, const uint32_t* traces) {      // the caller holds the batch
    if (b->single) {
        int rc = zk_trace_upload(b->single, traces, b->n - 1);
        if (rc) return rc;
        b->first[0] = traces[0]; b->last[0] = traces[b->n - 2];
        b->have_traces = true;
        return ZK_OK;
    }
    HIPCHK(hipSetDevice(b->device));
    for (size_t p = 0; p < b->batch * (b->n - 1); ++p)
        if (traces[p] >= P) return fail(ZK_ERR_INVALID, "zk_batch_set_traces: value %zu is not a canonical residue", p);
    HIPCHK(hipMemcpy2DAsync(b->d_trace, b->n * 4, traces, (b->n - 1) * 4, (b->n - 1) * 4, b->batch, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (size_t p = 0; p < b->batch; ++p) { b->first[p] = traces[p * (b->n - 1)]; b->last[p] = traces[p * (b->n - 1) + b->n - 2]; }
    b->have_traces = true;
    return ZK_OK;
}

// Fibonacci-square traces generated on the device from per-proof seeds (one lane per trace).
int zk_batch_gen_fibsq(zk_batch* b, const uint32_t* a0, const uint32_t* a1) {
    if (!b || !a0 || !a1) return fail(ZK_ERR_INVALID, "zk_batch_gen_fibsq: null argument");
    ZK_BATCH_EXCLUSIVE(b, "zk_batch_gen_fibsq");
    if (b->single) {                                       // prover.rs:32-39 is serial: one trace gains nothing from the device
        b->single_trace.resize(b->n - 1);
        int rc = zk_trace_fibsq(a0[0], a1[0], b->n - 1, b->single_trace.data());
        if (!rc) rc = set_traces_exclusive(b, b->single_trace.data());
        return rc;
    }
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpyAsync(b->d_seed, a0, b->batch * 4, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->d_seed + b->batch, a1, b->batch * 4, hipMemcpyHostToDevice, b->stream));
    HIPCHK(launch_trace_fibsq_batch(b->d_seed, b->d_seed + b->batch, (uint32_t)b->batch, (uint32_t)(b->n - 1), b->d_trace, b->stream, (uint32_t)b->n));
    // a[n-2] of every proof is a public input (prover.rs:42) and a constant of the second constraint
    HIPCHK(hipMemcpy2DAsync(b->h_last, 4, b->d_trace + (b->n - 2), b->n * 4, 4, b->batch, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (size_t p = 0; p < b->batch; ++p) { b->first[p] = a0[p] % P; b->last[p] = b->h_last[p]; }
    b->have_traces = true;
    return ZK_OK;
}

int zk_batch_public_last(const zk_batch* b, uint32_t* out) {
    if (!b || !out) return fail(ZK_ERR_INVALID, "zk_batch_public_last: null argument");
    if (!b->have_traces) return fail(ZK_ERR_STATE, "zk_batch_public_last: no traces");
    memcpy(out, b->last.data(), b->batch * 4);
    return ZK_OK;
}

// Nodes [first, first + count) of batch tree `tree` (a heap over batch * m_l leaves; proof p's tree is the subtree under node
// 2^log_batch - 1 + p).  Complete after zk_batch_prove: its last launches copy the host-built levels in (scatter_kernel).
// The log_batch levels ABOVE the per-proof roots belong to no proof and no launch builds them (MailArgs.top = log_batch): the nodes
// 0 .. 2^log_batch - 2 are hashed here, on the host, from the per-proof roots with the hash of the proof that built the tree.
// After a zk_batch_prove that FAILED (ZK_ERR_CHECK) the host-built levels were never copied in: the nodes are not that run's.
// A tree the last proof built with coset leaves of 2^steps values has m_l = len >> steps leaves per proof: its own, smaller heap.
int zk_batch_merkle_nodes(zk_batch* b, uint32_t tree, size_t first, size_t count, uint8_t* out) {
    if (!b || (!out && count)) return fail(ZK_ERR_INVALID, "zk_batch_merkle_nodes: null argument");
    if (b->single) return zk_merkle_nodes(b->single, tree, first, count, out);
    if (tree > b->R + 1) return fail(ZK_ERR_INVALID, "zk_batch_merkle_nodes: out of range");
    BusyScope busy(b);
    if (!busy.mine) return fail(ZK_ERR_STATE, "zk_batch_merkle_nodes: a zk_batch_prove is running on this batch");
    const size_t heap = 2 * (blayer_size(b, tree) >> b->tree_steps[tree]) * b->batch - 1;   // read under the flag: a running proof rewrites tree_steps
    if (first > heap || count > heap - first) return fail(ZK_ERR_INVALID, "zk_batch_merkle_nodes: out of range");
    if (tree == 0 && b->rows_tree0) return fail(ZK_ERR_STATE, "zk_batch_merkle_nodes: the last proof committed f as row leaves: tree 0 is not the batch's f heap");
    if ((b->skipped_trees >> tree) & 1)
        return fail(ZK_ERR_STATE, "zk_batch_merkle_nodes: tree %u was not built by the last proof (fold_log %u, fri_stop %u)", tree, b->proved_fold, b->proved_stop);
    if (count && b->tree_cap[tree] && first + 1 < ((size_t)1 << (b->lb + b->tree_cap[tree])))
        return fail(ZK_ERR_STATE, "zk_batch_merkle_nodes: node %zu of tree %u lies above its Merkle cap (depth %u): the last proof did not build it", first, tree,
                    b->lb + b->tree_cap[tree]);
    const uint32_t* d_heap = b->d_trees + b->tree_off[tree];
    const size_t top = b->batch - 1;                                      // nodes above the per-proof roots
    if (first >= top || !count) return merkle_nodes_to_host(b->device, b->stream, d_heap, first, count, out);
    std::vector<uint8_t> up((2 * b->batch - 1) * 32);
    if (int rc = merkle_nodes_to_host(b->device, b->stream, d_heap, top, b->batch, up.data() + 32 * top)) return rc;
    for (size_t i = top; i-- > 0;) host_node_hash(up.data() + 32 * (2 * i + 1), up.data() + 32 * (2 * i + 2), up.data() + 32 * i, b->proved_hash);
    const size_t n_top = count < top - first ? count : top - first;
    memcpy(out, up.data() + 32 * first, 32 * n_top);
    return merkle_nodes_to_host(b->device, b->stream, d_heap, first + n_top, count - n_top, out + 32 * n_top);
}

// What proof `proof` of the last zk_batch_prove committed for `tree`: the 2^ce digests of depth ce of its tree, nodes
// 2^(lb + ce) - 1 + proof 2^ce .. of the batch heap, which the device built or the scatter copied in (ce = 0: its root).
int zk_batch_merkle_cap(zk_batch* b, uint32_t tree, size_t proof, uint8_t* out, size_t out_len) {
    if (!b || !out) return fail(ZK_ERR_INVALID, "zk_batch_merkle_cap: null argument");
    if (b->single) return proof == 0 ? zk_ctx_merkle_cap(b->single, tree, out, out_len) : fail(ZK_ERR_INVALID, "zk_batch_merkle_cap: proof %zu out of range", proof);
    if (tree > b->R + 1) return fail(ZK_ERR_INVALID, "zk_batch_merkle_cap: tree %u out of range", tree);
    if (proof >= b->batch) return fail(ZK_ERR_INVALID, "zk_batch_merkle_cap: proof %zu out of range", proof);
    BusyScope busy(b);
    if (!busy.mine) return fail(ZK_ERR_STATE, "zk_batch_merkle_cap: a zk_batch_prove is running on this batch");
    if (!b->proved) return fail(ZK_ERR_STATE, "zk_batch_merkle_cap: no proof made yet");
    if (tree == 0 && b->rows_tree0) return fail(ZK_ERR_STATE, "zk_batch_merkle_cap: the last proof committed f as row leaves: tree 0 is not the batch's f heap");
    if ((b->skipped_trees >> tree) & 1)
        return fail(ZK_ERR_STATE, "zk_batch_merkle_cap: tree %u was not built by the last proof (fold_log %u, fri_stop %u)", tree, b->proved_fold, b->proved_stop);
    const uint32_t ce = b->tree_cap[tree];
    if (((size_t)32 << ce) > out_len) return fail(ZK_ERR_BUFFER, "zk_batch_merkle_cap: %zu bytes, room for %zu", (size_t)32 << ce, out_len);
    return merkle_nodes_to_host(b->device, b->stream, b->d_trees + b->tree_off[tree], (((size_t)1 << (b->lb + ce)) - 1) + (proof << ce), (size_t)1 << ce, out);
}

// generate_proof (prover.rs:9-293) for every resident trace: the run of the pipeline with 2^lb channels, every stage at width lb.
// proofs_out: [batch][stride] bytes, stride >= the length of the batch's format (zk_proof_data_len_* of its settings); states_out:
// [batch][32] (Channel.state of each proof, proof.rs:6).  Its own: every channel commits its own 2^ce digests of the f heap and draws
// its own alphas, on the pool; cp comes fused with its tree (prover.rs:166-176), or with coset leaves from its own launch under the tree
// with group 0's cosets as leaves.  A batch of one goes to the one-call prover.
int zk_batch_prove(zk_batch* b, uint8_t* proofs_out, size_t stride, uint8_t* states_out) {
    if (!b || !proofs_out || !states_out) return fail(ZK_ERR_INVALID, "zk_batch_prove: null argument");
    if (!b->have_traces) return fail(ZK_ERR_STATE, "zk_batch_prove: no traces");
    BusyScope busy(b);
    if (!busy.mine) return fail(ZK_ERR_STATE, "zk_batch_prove: another zk_batch_prove is running on this batch");
    const ProofFormat f = b->fmt;
    const size_t plen = f.data_len();
    if (stride < plen) return fail(ZK_ERR_BUFFER, "zk_batch_prove: stride %zu < proof length %zu", stride, plen);
    if (b->single) {
        size_t len = 0;
        int rc1 = zk_prove_resident(b->single, proofs_out, stride, &len, states_out);
        if (rc1 == ZK_ERR_CHECK) return fail(ZK_ERR_CHECK, "proof 0 of the batch: %s", last_error());
        return rc1;
    }
    HIPCHK(hipSetDevice(b->device));
    const size_t nb = b->batch;
    const uint32_t L = b->L, lb = b->lb;
    Run r{b, f, std::vector<Channel>(nb), lb, lb, "zk_batch_prove", 0};
    for (auto& c : r.ch) c.data.reserve(plen);
    r.T0 = now_us();
    int rc;
    ComposeBatchArgs ca;
    const uint32_t* roots;
    if ((rc = run_commit_f(r, 0, ca, &roots))) return rc;
    const uint32_t g2 = mulmod(b->dom->g, b->dom->g), ce = b->tree_cap[0];
    const double tc = btiming() ? now_us() : 0;
    b->pool->run(nb, 16, [&](size_t p) {
        commit_cap(r.ch[p], roots + ((p << ce) * 8), ce);
        if (f.ext) balphas_ext(b, p, r.ch[p], g2); else balphas(b, p, r.ch[p], g2);
    });
    cap_lap(r, ce, tc);
    if ((rc = bchal_upload(b, nb))) return rc;
    if (f.ext) {                                                          // both planes of cp from one pass over f, then the tree over them
        ca.a.cp = bext_layer(b, 1);
        HIPCHK(launch_compose_ext_batch(ca, b->d_xchal, (uint32_t)nb, b->stream, nullptr));
        if ((rc = btree(b, 1, L, f.slots_log(0), lb, true))) return rc;
    } else if (f.coset) {
        HIPCHK(launch_compose_batch(ca, lb, b->stream, nullptr));
        if ((rc = btree(b, 1, L, f.steps(0), lb))) return rc;
    } else {
        HIPCHK(launch_compose_merkle_batch(ca, lb, b->d_trees + b->tree_off[1], b->stream, nullptr, bmail(b, 1, L, lb), b->hash));
        if ((rc = bpost(b, 1, L, lb))) return rc;
    }
    if ((rc = run_groups(r)) || (rc = run_queries(r))) return rc;
    return run_decommit(r, proofs_out, stride, states_out);
}

// ONE proof of the batch's 2^log_batch resident traces (transcript.hpp "lb"): the run of the pipeline with one channel, whose
// FRI stage has width 0 -- proof 0's share of each layer slot and heap, row 0 of the challenge and final-polynomial tables -- over
// CP = sum_p cp_p.  Its own: the level the f heap hands over is committed once, 2^(lb + ce) digests; the one channel draws the 3 alphas of
// every statement; launch_compose_sum_batch writes CP into the first N words of layer 1 and its tree is built at width 0.  The gather
// buffers of the batch always hold a shared proof's openings (3M f tuples and one set of group tuples per query against M sets of both).
// Afterwards tree 0 is the batch's f heap as ever; the ids >= 1 hold one statement's worth and are reported as not built.
// Row leaves (zk_batch_set_shared_rows; transcript.hpp "rows"): the f stage has width 0 too -- ONE tree over the N rows of
// layer 0, handed over, posted and finished like cp's tree -- and a query opens three leaves of M slots in it.  Tree 0 is then that tree
// (2N - 1 nodes at tree_off[0]), not the batch's heap, and is reported as not built.
int zk_batch_prove_shared(zk_batch* b, uint8_t* proof_out, size_t cap, size_t* proof_len, uint8_t state_out[32]) {
    if (!b || !proof_out || !proof_len || !state_out) return fail(ZK_ERR_INVALID, "zk_batch_prove_shared: null argument");
    if (b->single || b->lb > kMaxSharedLog)
        return fail(ZK_ERR_INVALID, "zk_batch_prove_shared: need 1 <= log_batch <= %u (got %u): a batch of one makes a plain proof (zk_batch_prove)", kMaxSharedLog, b->lb);
    if (!b->have_traces) return fail(ZK_ERR_STATE, "zk_batch_prove_shared: no traces");
    BusyScope busy(b);
    if (!busy.mine) return fail(ZK_ERR_STATE, "zk_batch_prove_shared: another call (zk_batch_prove or a setter) is running on this batch");
    if (b->fmt.ext) return fail(ZK_ERR_STATE, "zk_batch_prove_shared: the batch has ext_log = 1 and a shared proof has no extension format (zk_batch_set_ext(b, 0) first)");
    ProofFormat f = b->fmt;
    f.lb = b->lb;
    f.rows = b->shared_rows;
    const size_t plen = f.data_len();
    *proof_len = plen;
    if (cap < plen) return fail(ZK_ERR_BUFFER, "zk_batch_prove_shared: buffer of %zu bytes < proof length %zu", cap, plen);
    size_t nv = 0, ndg = 0;                                               // values and digests a query opens
    bopenings(f, &nv, &ndg);
    if (nv + ndg > b->batch * (b->per_proof_vals + b->per_proof_digs) || nv + 8 * ndg > b->batch * (b->per_proof_vals + 8 * b->per_proof_digs))
        return fail(ZK_ERR_STATE, "zk_batch_prove_shared: gather buffers too small");
    HIPCHK(hipSetDevice(b->device));
    const uint32_t L = b->L, lb = b->lb;
    Run r{b, f, std::vector<Channel>(1), 0, f.rows ? 0 : lb, "zk_batch_prove_shared", 0};
    Channel& ch = r.ch[0];
    ch.data.reserve(plen);
    r.T0 = now_us();
    int rc;
    ComposeBatchArgs ca;
    const uint32_t* roots;
    if ((rc = run_commit_f(r, ~(uint64_t)1, ca, &roots))) return rc;      // only tree 0 is the batch's
    {
        const size_t count = ((size_t)1 << r.fw) << b->tree_cap[0];       // up to 2 MB in ONE commit: not on the stack
        std::vector<uint8_t> cb(32 * count);
        for (size_t i = 0; i < count; ++i) digest_words_to_bytes(roots + 8 * i, cb.data() + 32 * i);
        ch.commit_bytes(cb.data(), cb.size());
    }
    const uint32_t g2 = mulmod(b->dom->g, b->dom->g);
    for (size_t p = 0; p < b->batch; ++p) balphas(b, p, ch, g2);          // statement-major
    if ((rc = bchal_upload(b, b->batch))) return rc;
    HIPCHK(launch_compose_sum_batch(ca, lb, b->stream, nullptr));
    if ((rc = btree(b, 1, L, f.slots_log(0), 0))) return rc;
    if ((rc = run_groups(r)) || (rc = run_queries(r))) return rc;
    return run_decommit(r, proof_out, 0, state_out);
}

}  // extern "C"
