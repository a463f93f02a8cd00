// transcript.hpp -- host-only Fiat-Shamir channel, the proof wire format (one description for every folding factor, with one-value
// or coset leaves: length, opening order, decommitment tuple) and its verifier.
//
// Channel mirrors channel.rs:6-37; the byte encoding is bincode 1.x defaults
// (little-endian fixed-width ints, [u8;32] raw, Box<[T]> = u64 count + items)
// as read back by proof.rs:16-46.  The reference holds no golden bytes for the
// transcript, so this encoding is "parity unpinned" (SURVEY.md section 8c).
#pragma once
#include <stdint.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "../../include/zkstark_amd.h"
#include "blake2s.hpp"
#include "ext.hpp"
#include "field.hpp"
#include "fieldhash.hpp"
#include "sha256.hpp"

namespace zk {

struct Channel {
    uint8_t state[32];
    std::vector<uint8_t> data;
    Channel() { memset(state, 0, 32); }   // channel.rs:12-17
    // channel.rs:19-26
    void commit_bytes(const uint8_t* b, size_t n) {
        Sha256 h;
        h.update(state, 32);
        h.update(b, n);
        h.finalize(state);
        data.insert(data.end(), b, b + n);
    }
    void commit_hash(const uint8_t h[32]) { commit_bytes(h, 32); }
    void commit_u32(uint32_t v) {
        uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
        commit_bytes(b, 4);
    }
    // channel.rs:28-32
    uint32_t get_u32() {
        uint32_t f = ((uint32_t)state[0] << 24) | ((uint32_t)state[1] << 16) | ((uint32_t)state[2] << 8) | state[3];
        commit_u32(f);
        return f;
    }
    // The one decommitment tuple of the wire format: s values, then their s authentication paths, each Box<[Hash]> = u64 count +
    // plen digests, committed once.  s = 1 is (u32, AuthPath) of prover.rs:274-277, s = 2 the pair of prover.rs:280-289, s = 4 / 8
    // a group of a folded proof.  buf: group_bytes(s, plen) bytes of the caller's, reused from tuple to tuple; val(t) gives value
    // t, digest(i, out) writes digest i of the s * plen (path t starts at t * plen) as 32 bytes.
    // coset (coset leaves, below): the s values are the slots of ONE leaf, in slot order, and ONE path of plen digests follows them.
    static size_t group_bytes(size_t s, size_t plen, bool coset) { return 4 * s + (coset ? 1 : s) * (8 + 32 * plen); }
    // words: value words per opening (2 for values of E, "ext" below: val(t), t < s * words, in wire order); buf: that many bytes more
    template <class Val, class Dig> void commit_group(uint8_t* buf, size_t s, size_t plen, Val val, Dig digest, bool coset, uint32_t words = 1) {
        uint8_t* p = buf;
        for (size_t t = 0; t < s * words; ++t, p += 4) {
            const uint32_t v = val(t);
            for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
        }
        for (size_t t = 0; t < (coset ? 1 : s); ++t) {
            for (int i = 0; i < 8; ++i) *p++ = (uint8_t)((uint64_t)plen >> (8 * i));
            for (size_t j = 0; j < plen; ++j, p += 32) digest(t * plen + j, p);
        }
        commit_bytes(buf, (size_t)(p - buf));
    }
    // ... from values and paths that already lie as bytes (the sharded prover's decommitment): s = 1 and s = 2
    void commit_val_path(uint32_t val, const uint8_t* path, size_t plen) {
        std::vector<uint8_t> b(group_bytes(1, plen, false));
        commit_group(b.data(), 1, plen, [&](size_t) { return val; }, [&](size_t i, uint8_t* out) { memcpy(out, path + 32 * i, 32); }, false);
    }
    void commit_pair_paths(uint32_t v0, uint32_t v1, const uint8_t* p0, const uint8_t* p1, size_t plen) {
        std::vector<uint8_t> b(group_bytes(2, plen, false));
        commit_group(b.data(), 2, plen, [&](size_t t) { return t ? v1 : v0; },
                     [&](size_t i, uint8_t* out) { memcpy(out, i < plen ? p0 + 32 * i : p1 + 32 * (i - plen), 32); }, false);
    }
};

// ---- the proof format, in one place -----------------------------------------------------------------------------
// fold = K in 1..3 is the FRI folding factor 2^K (DESIGN.md "Folding factor"; the reference folds by two, K = 1: prover.rs:198-225).
// The R = log_n reference rounds are taken in G = ceil(R / K) groups; group j starts at round r0 = j K and has steps = min(K, R - r0)
// rounds.  A group draws ONE challenge beta; its output is `steps` successive reference folds with the challenges beta, beta^2,
// beta^4, and only that output is committed.  Per query a group opens the s = 2^steps values of its INPUT layer (len = N >> r0) at
// (x % len + t len / s) % len, t < s, then their s paths: the tuple of prover.rs:280-289 widened.  K = 1 is that tuple: G = R groups
// of one round, s = 2.  A query still tests one coset per layer, so the conjectured security per query is the reference's; the
// price of K > 1 is s paths per group instead of 2 per round.
// q = number of decommitment queries (1 = the reference's format, prover.rs:263; q > 1: SURVEY.md 8f item 1 -- the q raw indices
// are drawn in a row, then each query's openings are committed in turn).
// grind = proof-of-work bits (DESIGN.md "Grinding"): g > 0 puts the 8-byte nonce between the free term and the query raws.
// coset = coset leaves (off = the format above).  The tree over the input layer of group j (id 1 + r0, len = N >> r0,
// s = 2^steps_j) has len / s leaves; leaf c holds the slots u = 0 .. s-1, slot u = layer[c + u len / s] (the layer itself stays in
// natural order): exactly what a query opens there, so a group is ONE leaf and ONE path of L - r0 - steps digests for leaf
// x % (len / s).  Leaf hash: SHA-256 over the s slots, 4 bytes big-endian each (one block); BLAKE2s-256 over the same message
// (blake2s.hpp); field hash: the compression of (slot_0 .. slot_{s-1}, 0, ..., 0, s) (fieldhash.hpp).  s = 1 is the one-value leaf.  Inner nodes are unchanged; tree 0 (f) and
// the tree over the last layer (id 1 + log_n, never opened) keep one-value leaves.  Per query the three f tuples are sent as ever;
// the separate cp(x) tuple is dropped (group 0's leaf contains it), then per group the s slot values in slot order, a u64 count and
// the path.  With rot = (x % len) / (len / s), value t of the group (the one at (x % len + t len / s) % len) is slot (rot + t) % s.
// stop = D in 0..kMaxStopLog is the early stop (DESIGN.md 7d "Early stop"; 0 = fold down to a constant, the format above).  Only the
// first R' = log_n - D rounds are folded, in the groups of R' (G' of them); the output of the last group, layer id 1 + R', holds
// M = 2^(D + log_b) evaluations of a polynomial p of degree < 2^D at X_i = (w h^i)^(2^R').  It gets no tree: in place of the last root
// and the free term the header carries the 2^D monomial coefficients of p in X (canonical residues, 4 bytes little-endian each,
// ONE commit), then the nonce and the query raws as ever.  Per query the tuples of the G' groups are sent unchanged, and the last
// group's fold is compared with p(x^(2^R')), evaluated by Horner.  A query still tests one coset per committed layer, and the
// degree bound of the final polynomial holds by construction (2^D coefficients ARE a polynomial of degree < 2^D).
constexpr uint32_t kMaxFoldLog = 3;
constexpr uint32_t kMaxStopLog = 8, kMaxStopLayerLog = 12;   // the stopped layer (2^(D + log_b) values) fits one workgroup's LDS
constexpr uint32_t kMaxGrindBits = 32;
// D = 0, or 1 <= D <= 8 with at least one folded round and a stopped layer of at most 2^12 values
inline bool stop_ok(uint32_t log_n, uint32_t log_b, uint32_t stop) {
    return stop == 0 || (stop <= kMaxStopLog && stop + 1 <= log_n && stop + log_b <= kMaxStopLayerLog);
}
// Leaf t of the coset a group with `steps` rounds opens in its input layer of 2^log_len values, for the query index x.
inline size_t coset_leaf(size_t x, uint32_t log_len, uint32_t steps, uint32_t t) {
    const size_t len = (size_t)1 << log_len;
    return (x % len + t * (len >> steps)) % len;
}
// cap = c in 0..kMaxCapLog, Merkle caps: a tree over 2^lg leaves (coset leaves count as one) is committed by the 2^ce
// digests of depth ce = min(c, lg - 1) -- heap nodes 2^ce - 1 .. 2^(ce+1) - 2, left to right, 32 bytes each, ONE commit -- in place of
// its root, and a path into it carries the lg - ce siblings from the leaf up to depth ce + 1 (the u64 count in front is lg - ce).  The
// verifier hashes upward lg - ce times and compares with cap entry leaf >> (lg - ce).  ce = 0 is the root: a cap-0 proof is the format
// above, byte for byte.  Every committed tree takes part: f, the tree over every group's input layer, and the never-opened last tree
// when stop = 0.  A path that misses its cap entry gets the check number it gets for missing the root.  verify_proof tests only the
// entries a path lands in; a changed entry that no path lands in is caught by verify_transcript alone (the challenge after it, as for a
// changed root).
constexpr uint32_t kMaxCapLog = 8;
// lb = log_batch in 0..kMaxSharedLog, the shared proof: ONE proof of M = 2^lb statements of one size, statement p being
// fibsq with its own public_last[p].  lb = 0 is the format above, byte for byte.  The M trace polynomials f_p are committed together: the
// header opens with the 2^(lb + ce_f) digests of depth lb + ce_f of the heap over all M f layers (statement p's cap: entries p 2^ce_f
// onwards; ONE commit), then 3M alphas, statement-major.  From cp on the header is a single proof's, over CP = sum_p cp_p (mod P), cp_p
// the composition of statement p with its own three alphas and its own public_last.  Per query the three f tuples of statement 0, then
// of statement 1, ... (each a value and f_path() digests into statement p's subtree), then the cp tuple and the group tuples as ever.
// verify_proof: -2 compares sum_p (alpha0_p p0_p + alpha1_p p1_p + alpha2_p p2_p) at x with the cp value opened; -3 covers the 3M f path
// lengths (and cp's); -4 / -5 / -6 the path of f_p(x) / f_p(gx) / f_p(g^2 x) of the first failing tuple in wire order; the rest as ever.
// verify_transcript counts 3M + G + q challenges; 3 * 256 + 30 + 64 keeps -(1000 + k) clear of -1998.
constexpr uint32_t kMaxSharedLog = 8;
// rows = row leaves of a shared proof (needs 1 <= lb; off = the format above).  The M trace polynomials are committed as ONE
// tree over N leaves, leaf i holding the row (f_0[i], .., f_{M-1}[i]): the proof-major array [M][N] read as one layer of M N values whose
// leaves hold 2^lb slots, slot u = layer[i + u N].  The header opens with that tree's cap, the 2^ce_f digests of depth ce_f = min(c, L - 1)
// (ONE commit; cap 0: one root), then the 3M alphas as ever.  Per query three tuples -- the rows x, x + B, x + 2B -- each the M values of the
// row in statement order, a u64 count and ONE path of L - ce_f digests; then the cp tuple and the group tuples as ever.  Leaf hash of a row
// (host_coset_leaf_hash with s = M): SHA-256 of the 4M-byte message, 4 bytes big-endian per value (M <= 8: the coset leaf's one block;
// M >= 16: M / 16 data blocks and one padding block); field hash: fieldhash_row_leaf (fieldhash.hpp; M <= 8: the coset leaf, M >= 16 a chain
// of M / 8 compressions).  No BLAKE2s: no prover makes such a proof.  verify_proof: -2 as ever (f_p(x) is value p of row x); -3 covers the
// three row path lengths (and cp's); -4 / -5 / -6 the path of row x / x + B / x + 2B against cap entry leaf >> (L - ce_f).  The length is a
// single proof's plus 12 (M - 1) (1 + q): the further alphas and 4 (M - 1) more value bytes in each of the 3 q row tuples.
// ext = 1, challenges in the quadratic extension E = F_P[u] / (u^2 - 5) (ext.hpp; 0 = the format above, byte for byte; needs lb = 0).
// The trace and f stay in the base field; the alphas, cp, every beta and every FRI layer are in E.  A challenge is two get_u32 draws in a row,
// c0 then c1: the alphas are alpha0.c0, alpha0.c1, alpha1.c0, .. (24 bytes), a group's beta 8 bytes.  cp = alpha0 p0 + alpha1 p1 + alpha2 p2 with
// the base-field quotients, so component j of cp is the base composition with the component-j alphas; a group folds with beta, beta^2, beta^4
// squared in E, the points in the base field.  The leaf over the slots u < S of a layer with id >= 1 holds 2 S words, the S component-0 words in
// slot order, then the S component-1 words, hashed as a row of 2 S values (host_coset_leaf_hash; no BLAKE2s); the never-opened last tree has
// leaves of 2 words.  On the wire every cp or group tuple sends, where it sent s value words, 2 s: the s component-0 words, then the s
// component-1 words; counts and paths as ever, the three f tuples unchanged.  kFinal: c0 then c1 of the free term (8 bytes), or the 2^stop
// component-0 coefficients, then the 2^stop component-1 coefficients.  verify_proof_ext keeps verify_proof's check numbers one for one; a
// comparison of values of E fails when either component differs.  verify_transcript counts 6 + 2G + q challenges.  Another length: -1.
inline uint32_t cap_eff(uint32_t cap, uint32_t lg) { return cap < lg - 1 ? cap : lg - 1; }   // lg >= 1 for every committed tree

// One proof format: the settings above and everything that follows from them.  The Merkle hash and public_last are not part of it.
// The wire order is written down twice, here and nowhere else: for_each_head (the header) and for_each_tuple (one query); lengths,
// provers and verifiers walk those.  A new setting is a field and a line in a walk.
struct ProofFormat {
    uint32_t log_n = 0, log_b = 0, q = 1, grind = 0, fold = 1;
    bool coset = false;
    uint32_t stop = 0, cap = 0;
    uint32_t lb = 0;                                                         // shared proof of 2^lb statements (0: a plain proof)
    bool rows = false;                                                       // ... whose f values are committed as row leaves (needs lb >= 1)
    uint32_t ext = 0;                                                        // challenges, cp and the FRI layers in the extension of degree 2^ext (0 or 1)

    // what verify_proof and verify_transcript take (they answer -1 to anything else); every member below assumes it
    bool ok() const {
        return log_n >= 2 && log_b >= 1 && log_n + log_b <= 30 && q >= 1 && q <= 64 && grind <= kMaxGrindBits && fold >= 1 && fold <= kMaxFoldLog &&
               stop_ok(log_n, log_b, stop) && cap <= kMaxCapLog && lb <= kMaxSharedLog && (!rows || lb >= 1) && ext <= 1 && (!ext || lb == 0);
    }
    // ---- geometry.  Group j < G folds the rounds round0(j) .. round0(j) + steps(j) - 1; tree j is the one over its INPUT layer.
    // j = G: the last layer (round0 = rounds, steps = 0), whose tree has one-value leaves and exists only when stop = 0.
    uint32_t L() const { return log_n + log_b; }
    uint32_t rounds() const { return log_n - stop; }                         // the folded rounds R'
    uint32_t groups() const { return (rounds() + fold - 1) / fold; }
    uint32_t round0(uint32_t j) const { return j * fold < rounds() ? j * fold : rounds(); }
    uint32_t steps(uint32_t j) const { return rounds() - round0(j) < fold ? rounds() - round0(j) : fold; }
    uint32_t tree_id(uint32_t j) const { return 1 + round0(j); }             // layer and tree ids: 0 = f, 1 = cp, 1 + r = after r rounds
    uint32_t slots_log(uint32_t j) const { return coset ? steps(j) : 0; }    // log2 of the values per leaf of tree j
    uint32_t tree_log(uint32_t j) const { return L() - round0(j) - slots_log(j); }   // log2 of its leaf count
    bool last_tree() const { return stop == 0; }
    uint32_t f_cap() const { return cap_eff(cap, L()); }                     // the depth a tree is committed at ...
    uint32_t tree_cap(uint32_t j) const { return cap_eff(cap, tree_log(j)); }
    size_t f_path() const { return (size_t)L() - f_cap(); }                  // ... and the digests of a path into it
    size_t tree_path(uint32_t j) const { return (size_t)tree_log(j) - tree_cap(j); }

    // ---- the header in wire order: fn(what, j, bytes) -> bool, false ends the walk (and is returned).  kAlphas, kBeta and kRaws are
    // challenges of 4 bytes each (3 per statement, 1 and q of them), everything else is ONE commit.  kTree j: the commitment of tree j.
    // kFTree: the caps of all 2^lb statements' f trees, statement-major, in one commit; rows: the cap of the one tree over the rows.
    enum Head { kFTree, kAlphas, kTree, kBeta, kFinal, kNonce, kRaws };
    template <class Fn> bool for_each_head(Fn fn) const {
        const uint32_t G = groups();
        if (!fn(kFTree, 0u, (size_t)32 << ((rows ? 0 : lb) + f_cap())) || !fn(kAlphas, 0u, (size_t)12 << (lb + ext)) || !fn(kTree, 0u, (size_t)32 << tree_cap(0))) return false;
        for (uint32_t j = 0; j < G; ++j) {
            if (!fn(kBeta, j, (size_t)4 << ext)) return false;                     // group j's challenge, then the tree over its output
            if ((j + 1 < G || last_tree()) && !fn(kTree, j + 1, (size_t)32 << tree_cap(j + 1))) return false;
        }
        if (!fn(kFinal, 0u, (size_t)4 << (stop + ext))) return false;           // the free term, or the 2^stop coefficients (ext: per component)
        if (grind && !fn(kNonce, 0u, (size_t)8)) return false;
        return fn(kRaws, 0u, (size_t)4 * q);
    }
    // ---- the tuples of one query in wire order: fn(s values, digests per path, one_leaf) as Channel::commit_group takes them.
    // f(x), f(gx), f(g^2 x) of every statement (rows: the three rows of 2^lb values, one leaf each) and, with one-value leaves, cp(x);
    // then one tuple per group.  A walker that knows of ext takes a fourth argument, the words per value of the tuple (1 for the f tuples,
    // 2^ext for cp and the groups: tuple_bytes); the provers and the GPU verifier, which have no such setting, take three.
    template <class Fn> static void tuple(Fn& fn, size_t s, size_t plen, bool one_leaf, uint32_t words) {
        if constexpr (std::is_invocable_v<Fn&, size_t, size_t, bool, uint32_t>) fn(s, plen, one_leaf, words);
        else fn(s, plen, one_leaf);
    }
    static size_t tuple_bytes(size_t s, size_t plen, bool one_leaf, uint32_t words) { return Channel::group_bytes(s, plen, one_leaf) + 4 * s * (words - 1); }
    template <class Fn> void for_each_tuple(Fn fn) const {
        if (rows) for (int k = 0; k < 3; ++k) tuple(fn, (size_t)1 << lb, f_path(), true, 1u);
        else for (size_t i = 0; i < ((size_t)3 << lb); ++i) tuple(fn, (size_t)1, f_path(), false, 1u);
        if (!coset) tuple(fn, (size_t)1, tree_path(0), false, 1u << ext);
        for (uint32_t j = 0, G = groups(); j < G; ++j) tuple(fn, (size_t)1 << steps(j), tree_path(j), coset, 1u << ext);
    }
    // ---- the openings of one query in the same order, for x = query raw % (N - 2B): f at x, x + B, x + 2B (layer 0) and cp at x
    // (layer 1) (prover.rs:266-277), then per group the s coset leaves of its input layer.  An opening is one LEAF and its path:
    // open(layer id, log2 of the tree's leaf count, leaf index, slots_log); the leaf holds the 2^slots_log values
    // layer[leaf + u 2^(log2 leaf count)], u < 2^slots_log (0: a one-value leaf).  Both provers rely on this leaf order.
    // Shared proof: statement p's f openings are the leaves (p << L) + x .. of layer 0, i.e. of the proof-major [2^lb][N] array; rows:
    // the leaves x, x + B, x + 2B of the tree over that array's N rows, 2^lb slots each.
    template <class Open> void for_each_opening(size_t x, Open open) const {
        const size_t B = (size_t)1 << log_b;
        if (rows) { open(0u, L(), x, lb); open(0u, L(), x + B, lb); open(0u, L(), x + 2 * B, lb); }
        else for (size_t p = 0; p < ((size_t)1 << lb); ++p) {
            const size_t at = (p << L()) + x;
            open(0u, L(), at, 0u); open(0u, L(), at + B, 0u); open(0u, L(), at + 2 * B, 0u);
        }
        if (!coset) open(1u, L(), x, 0u);
        for (uint32_t j = 0, G = groups(); j < G; ++j) {
            const uint32_t lg = tree_log(j), st = steps(j);
            if (coset) open(tree_id(j), lg, x % ((size_t)1 << lg), st);
            else for (uint32_t t = 0; t < (1u << st); ++t) open(tree_id(j), lg, coset_leaf(x, lg, st, t), 0u);
        }
    }
    // bytes of a proof: the header, then q queries
    size_t data_len() const {
        size_t head = 0, per_query = 0;
        for_each_head([&](Head, uint32_t, size_t bytes) { head += bytes; return true; });
        for_each_tuple([&](size_t s, size_t plen, bool one_leaf, uint32_t words) { per_query += tuple_bytes(s, plen, one_leaf, words); });
        return head + (size_t)q * per_query;
    }
};

// ---- grinding (DESIGN.md "Grinding"; the reference has none) -------------------------------------------------------------
// After the free term, with channel state S, the prover commits le64(w) for the smallest w >= 0 such that SHA-256(S || le64(w))
// starts with g zero bits (MSB-first from byte 0, as get_u32 reads the state).  The commit itself computes that hash, so the
// bits are those of the channel state right after the nonce is committed.
constexpr uint64_t kGrindLimit = (uint64_t)1 << 44;      // a search gives up after this many nonces
// Digest word 0 of SHA-256(state || le64(w)): one compression of a single block.
inline uint32_t grind_word0(const uint8_t state[32], uint64_t w) {
    uint32_t blk[16] = {0};
    for (int i = 0; i < 8; ++i)
        blk[i] = ((uint32_t)state[4 * i] << 24) | ((uint32_t)state[4 * i + 1] << 16) | ((uint32_t)state[4 * i + 2] << 8) | state[4 * i + 3];
    blk[8] = __builtin_bswap32((uint32_t)w);
    blk[9] = __builtin_bswap32((uint32_t)(w >> 32));
    blk[10] = 0x80000000u;
    blk[15] = 320u;                                       // 40 bytes
    uint32_t st[8];
    for (int i = 0; i < 8; ++i) st[i] = SHA_IV[i];
    host_sha_compress(st, blk);
    return st[0];
}
inline bool grind_word_ok(uint32_t word0, uint32_t bits) { return bits == 0 || (word0 >> (32 - bits)) == 0; }
inline void grind_commit(Channel& ch, uint64_t w) {
    uint8_t b[8];
    for (int i = 0; i < 8; ++i) b[i] = (uint8_t)(w >> (8 * i));   // bincode u64
    ch.commit_bytes(b, 8);
}

// Merkle hash on the host (verifier), a zk_hash_kind: SHA-256 (merkle.rs:30-34, :42-45), field-native (fieldhash.hpp) or
// BLAKE2s-256 (blake2s.hpp).  The channel and the grinding hash above are SHA-256 whatever the Merkle hash.
inline const FieldHashConsts& host_fieldhash_consts() {
    static const FieldHashConsts c = [] { FieldHashConsts t; fieldhash_make_consts(t); return t; }();
    return c;
}
inline void bytes_to_digest(const uint8_t* b, Digest& d) {
    for (int i = 0; i < 8; ++i) d.w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
}
inline void host_leaf_hash(uint32_t element, uint8_t out[32], int hash) {
    if (hash == ZK_HASH_BLAKE2S) { digest_words_to_bytes(blake2s_leaf(element).w, out); return; }
    if (hash == ZK_HASH_FIELD) { digest_words_to_bytes(fieldhash_leaf(element, host_fieldhash_consts()).w, out); return; }
    uint8_t be[4] = {(uint8_t)(element >> 24), (uint8_t)(element >> 16), (uint8_t)(element >> 8), (uint8_t)element};
    Sha256 h; h.update(be, 4); h.finalize(out);
}
inline void host_node_hash(const uint8_t* l, const uint8_t* r, uint8_t out[32], int hash) {
    if (hash != ZK_HASH_SHA256) {
        Digest dl, dr;
        bytes_to_digest(l, dl); bytes_to_digest(r, dr);
        digest_words_to_bytes((hash == ZK_HASH_BLAKE2S ? blake2s_inner(dl, dr) : fieldhash_inner(dl, dr, host_fieldhash_consts())).w, out);
        return;
    }
    Sha256 h; h.update(l, 32); h.update(r, 32); h.finalize(out);
}

// Leaf of s <= 8 slots (coset leaves, above; s = 1 is host_leaf_hash) or of a row of s <= 2^kMaxSharedLog values (row leaves, above: a
// power of two; SHA-256 and the field hash only -- a BLAKE2s leaf has at most 8 slots).
inline void host_coset_leaf_hash(const uint32_t* slots, size_t s, uint8_t out[32], int hash) {
    if (hash == ZK_HASH_BLAKE2S) { digest_words_to_bytes(blake2s_coset_leaf(slots, s < 8 ? s : 8).w, out); return; }
    if (hash == ZK_HASH_FIELD) { digest_words_to_bytes(fieldhash_row_leaf(slots, (uint32_t)s, host_fieldhash_consts()).w, out); return; }
    uint8_t be[4 << kMaxSharedLog];
    if (s > ((size_t)1 << kMaxSharedLog)) s = (size_t)1 << kMaxSharedLog;
    for (size_t u = 0; u < s; ++u) { be[4 * u] = (uint8_t)(slots[u] >> 24); be[4 * u + 1] = (uint8_t)(slots[u] >> 16); be[4 * u + 2] = (uint8_t)(slots[u] >> 8); be[4 * u + 3] = (uint8_t)slots[u]; }
    Sha256 h; h.update(be, 4 * s); h.finalize(out);
}

// merkle.rs:82-110, from the s slots of leaf `index` (s = 1: the reference's one element)
inline void compute_root_from_coset(const uint32_t* slots, size_t s, size_t index, const uint8_t* path, size_t plen, uint8_t out[32], int hash = 0) {
    index += ((size_t)1 << plen) - 1;
    uint8_t cur[32], nxt[32];
    host_coset_leaf_hash(slots, s, cur, hash);
    for (size_t k = 0; k < plen; ++k) {
        if (index % 2 == 0) { host_node_hash(path + 32 * k, cur, nxt, hash); index -= 2; }
        else { host_node_hash(cur, path + 32 * k, nxt, hash); index -= 1; }
        memcpy(cur, nxt, 32);
        index >>= 1;
    }
    memcpy(out, cur, 32);
}
inline void compute_root_from_path(uint32_t element, size_t index, const uint8_t* path, size_t plen, uint8_t out[32], int hash = 0) {
    compute_root_from_coset(&element, 1, index, path, plen, out, hash);
}

// proof.rs:15-149 with the literals generalised and the rounds taken in groups (the format above).  Returns 0 or the negative
// index of the failed check: -1 sizes or layout, -2 cp0, -3 the four path lengths, -4..-7 the paths of f(x), f(gx), f(g^2 x), cp(x);
// then per query first every group's fold comparison -(100+j), then per group j its path lengths -(200+j) and its paths,
// -(300+j) for t = 0 and -(400+j) for the first failing t >= 1; -8 for bytes left over.  K = 1: j is the reference's round.
// Values and challenges are reduced % P before arithmetic; what a fold is compared with (the next group's value 0, the free
// term, fv[3]) is compared unreduced.
// coset: cp0 is compared with group 0's value 0 (-2), -3 covers the three f path lengths, -7 and -(400+j) do not occur: a group has
// one path length -(200+j) and one path -(300+j).
// grind > 0: the nonce after the free term is skipped.  Its work is a property of the Fiat-Shamir transcript, which only
// verify_transcript replays; here the query raws are read from the proof (as the reference does), so checking it certifies nothing.
// stop > 0 (early stop, above): the groups are those of log_n - stop rounds, the header ends with the 2^stop coefficients in place of
// the last root and the free term, and the last group's fold -(100 + (G' - 1)) is compared with p(x^(2^R')) -- Horner over the
// coefficients, each reduced % P on reading, as raw challenges are.
// cap > 0 (Merkle caps, above): every root of the header is 2^ce digests, the path lengths expected are lg - ce, and a path is
// compared with the cap entry it lands in, under the check number it has for the root.  A proof of another length: -1.
// lb > 0 (the shared proof, above): public_last holds 2^lb values; the f tuples are 3 per statement, fv[3 p + k], and the cp value is
// fv[3 M].  lb = 0: one statement, fv[0..3] as ever.
// rows (row leaves, above): three f tuples of M values each, row k at fv[k M ..]; f_p at x + k B is fv[k M + p].  BLAKE2s: -1.
inline int verify_proof_ext(const uint8_t* data, size_t len, const ProofFormat& fmt, uint32_t public_last, int hash);
inline int verify_proof(const uint8_t* data, size_t len, const ProofFormat& fmt, const uint32_t* public_last, int hash) {
    if (!fmt.ok() || (fmt.rows && hash == ZK_HASH_BLAKE2S)) return -1;
    if (fmt.ext) return verify_proof_ext(data, len, fmt, public_last[0], hash);   // ext = 0 is the code below, untouched
    if ((fmt.stop || fmt.cap || fmt.lb) && len != fmt.data_len()) return -1;   // a stopped, capped or shared proof of another length: -1, strict or not
    const bool coset = fmt.coset;
    const size_t M = (size_t)1 << fmt.lb;
    const bool rows = fmt.rows;
    const uint32_t ncp = 3 * (uint32_t)M;                               // f(x), f(gx), f(g^2 x) per statement: the f values of a query
    const uint32_t nft = rows ? 3 : ncp, nf = nft + (coset ? 0 : 1);    // ... in nft tuples; nf with the cp(x) tuple of one-value leaves
    const size_t n = (size_t)1 << fmt.log_n, B = (size_t)1 << fmt.log_b, N = n << fmt.log_b;
    const uint32_t L = fmt.L(), G = fmt.groups();
    const uint8_t* p = data;
    size_t left = len;
    bool bad = false;
    auto take = [&](size_t k) -> const uint8_t* {
        if (left < k) { bad = true; return nullptr; }
        const uint8_t* r = p; p += k; left -= k; return r;
    };
    auto take32 = [&]() -> uint32_t {
        const uint8_t* r = take(4);
        return r ? ((uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24)) : 0;
    };
    auto take_path = [&](size_t& plen) -> const uint8_t* {
        const uint8_t* r = take(8);
        if (!r) return nullptr;
        uint64_t c = 0;
        for (int i = 0; i < 8; ++i) c |= (uint64_t)r[i] << (8 * i);
        if (c > 64) { bad = true; return nullptr; }
        plen = (size_t)c;
        return take(32 * plen);
    };
    auto le32 = [](const uint8_t* r) { return (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24); };
    // proof.rs:20-46.  roots[j]: the commitment of the tree over the INPUT layer of group j (roots[G]: the last layer)
    const uint8_t *f_root = nullptr, *alphas = nullptr, *final_term = nullptr, *raws = nullptr, *roots[41] = {nullptr}, *betas[40];
    fmt.for_each_head([&](ProofFormat::Head what, uint32_t j, size_t bytes) {
        const uint8_t* r = take(bytes);
        switch (what) {
            case ProofFormat::kFTree: f_root = r; break;
            case ProofFormat::kAlphas: alphas = r; break;
            case ProofFormat::kTree: roots[j] = r; break;
            case ProofFormat::kBeta: betas[j] = r; break;
            case ProofFormat::kFinal: final_term = r; break;   // the free term, or the coefficients
            case ProofFormat::kNonce: break;
            case ProofFormat::kRaws: raws = r; break;
        }
        return true;
    });
    if (bad) return -1;
    const uint32_t g = root_of_unity(fmt.log_n), h = root_of_unity(L);
    for (uint32_t qk = 0; qk < fmt.q; ++qk) {
        uint32_t fv[3 * (1u << kMaxSharedLog) + 1]; const uint8_t* fp[3 * (1u << kMaxSharedLog) + 1]; size_t fpl[3 * (1u << kMaxSharedLog) + 1];
        for (uint32_t t = 0; t <= nft; ++t) fpl[t] = 0;
        uint32_t lv[40][8]; const uint8_t* lp[40][8]; size_t lpl[40][8];
        uint32_t i = 0;                                      // tuple i: an f / cp tuple, then group i - nf
        fmt.for_each_tuple([&](size_t s, size_t, bool one_leaf) {
            uint32_t* v = i < nf ? &fv[!rows ? i : i < 3 ? i * M : ncp] : lv[i - nf];   // the cp value is fv[3 M] either way
            const uint8_t** path = i < nf ? &fp[i] : lp[i - nf];
            size_t* plen = i < nf ? &fpl[i] : lpl[i - nf];
            for (size_t t = 0; t < s; ++t) v[t] = take32();
            for (size_t t = 0; t < (one_leaf ? 1 : s); ++t) { plen[t] = 0; path[t] = take_path(plen[t]); }
            ++i;
        });
        if (bad) return -1;
        // proof.rs:49-60
        const size_t tp = (size_t)le32(raws + 4 * qk) % (N - 2 * B);
        // value t of group j: as sent, or slot (rot + t) % s of the group's leaf
        auto group_val = [&](uint32_t j, uint32_t t) -> uint32_t {
            if (!coset) return lv[j][t];
            const uint32_t steps = fmt.steps(j), lg = L - fmt.round0(j);
            const size_t rot = (tp & (((size_t)1 << lg) - 1)) >> (lg - steps);
            return lv[j][(rot + t) & ((1u << steps) - 1u)];
        };
        if (coset) fv[ncp] = group_val(0, 0);
        const uint32_t x = mulmod(GEN_W, powmod(h, tp));
        {   // proof.rs:63-77, summed over the statements (the denominators depend on x alone)
            const uint32_t gm1 = invmod(g), gm2 = mulmod(gm1, gm1), gm3 = mulmod(gm2, gm1);
            const uint32_t i0 = invmod(sub(x, 1)), i1 = invmod(sub(x, gm2));
            const uint32_t den = mulmod(sub(powmod(x, n), 1), invmod(mulmod(mulmod(sub(x, gm3), sub(x, gm2)), sub(x, gm1))));
            const uint32_t i2 = invmod(den);
            uint32_t cp0 = 0;
            for (size_t s = 0; s < M; ++s) {
                const uint8_t* al = alphas + 12 * s;
                const size_t at = rows ? s : 3 * s, step = rows ? M : 1;
                uint32_t f_x = fv[at] % P, f_gx = fv[at + step] % P, f_ggx = fv[at + 2 * step] % P;
                uint32_t p0 = mulmod(sub(f_x, 1), i0);
                uint32_t p1 = mulmod(sub(f_x, public_last[s] % P), i1);
                uint32_t num = sub(sub(f_ggx, mulmod(f_gx, f_gx)), mulmod(f_x, f_x));
                uint32_t p2 = mulmod(num, i2);
                cp0 = add(cp0, add(add(mulmod(le32(al) % P, p0), mulmod(le32(al + 4) % P, p1)), mulmod(le32(al + 8) % P, p2)));
            }
            if (cp0 != fv[ncp]) return -2;
        }
        uint8_t root[32];
        // the path of leaf `idx` (s slots) climbs plen levels and must land on entry idx >> plen of the tree's cap (cap 0: on the root)
        auto misses = [&](const uint32_t* slots, size_t s, size_t idx, const uint8_t* path, size_t plen, const uint8_t* entries) -> bool {
            compute_root_from_coset(slots, s, idx & (((size_t)1 << plen) - 1), path, plen, root, hash);
            return memcmp(root, entries + 32 * (idx >> plen), 32) != 0;
        };
        for (uint32_t k = 0; k < nft; ++k) if (fpl[k] != fmt.f_path()) return -3;
        if (!coset && fpl[nft] != fmt.tree_path(0)) return -3;
        // proof.rs:80-95; statement s's paths land in its own 2^ce entries of the f commitment (rows: row k is ONE leaf of M slots)
        for (uint32_t k = 0; rows && k < 3; ++k)
            if (misses(&fv[k * M], M, tp + k * B, fp[k], fpl[k], f_root)) return -(int)(4 + k);
        for (size_t s = 0; !rows && s < M; ++s) {
            const uint8_t* cap_s = f_root + ((size_t)32 << fmt.f_cap()) * s;
            if (misses(&fv[3 * s], 1, tp, fp[3 * s], fpl[3 * s], cap_s)) return -4;
            if (misses(&fv[3 * s + 1], 1, tp + B, fp[3 * s + 1], fpl[3 * s + 1], cap_s)) return -5;
            if (misses(&fv[3 * s + 2], 1, tp + 2 * B, fp[3 * s + 2], fpl[3 * s + 2], cap_s)) return -6;
        }
        if (!coset && misses(&fv[ncp], 1, tp, fp[nft], fpl[nft], roots[0])) return -7;
        // proof.rs:101-126: the s opened values of a group folded pairwise (t with t + s/2, then again)
        const uint32_t inv2 = invmod(2);
        for (uint32_t j = 0; j < G; ++j) {
            const uint32_t r0 = fmt.round0(j), steps = fmt.steps(j);
            uint32_t cnt = 1u << steps, v[8];
            for (uint32_t t = 0; t < cnt; ++t) v[t] = group_val(j, t) % P;
            uint32_t xk = powmod(x, (uint64_t)1 << r0);                        // the point of index tp % len in layer r0
            uint32_t om = powmod(h, (uint64_t)N >> steps);                     // index + len / s: the point times a primitive s-th root of unity
            uint32_t bk = le32(betas[j]) % P;
            for (uint32_t k = 0; k < steps; ++k) {
                cnt >>= 1;
                uint32_t pt = xk;
                for (uint32_t t = 0; t < cnt; ++t) {
                    const uint32_t gx = mulmod(add(v[t], v[t + cnt]), inv2);
                    const uint32_t hx = mulmod(sub(v[t], v[t + cnt]), invmod(mulmod(pt, 2)));
                    v[t] = add(gx, mulmod(bk, hx));
                    pt = mulmod(pt, om);
                }
                xk = mulmod(xk, xk); om = mulmod(om, om); bk = mulmod(bk, bk);
            }
            uint32_t expect = (j + 1 < G) ? group_val(j + 1, 0) : fmt.stop ? 0 : le32(final_term);
            if (fmt.stop && j + 1 == G) {                                      // p at the point of the stopped layer, x^(2^R')
                const uint32_t xs = powmod(x, (uint64_t)1 << fmt.rounds());
                for (size_t k = (size_t)1 << fmt.stop; k-- > 0; ) expect = add(mulmod(expect, xs), le32(final_term + 4 * k) % P);
            }
            if (v[0] != expect) return -(int)(100 + j);
        }
        // proof.rs:129-148
        for (uint32_t j = 0; j < G; ++j) {
            const uint32_t lg = fmt.tree_log(j), steps = fmt.steps(j), s = 1u << steps;
            if (coset) {
                if (lpl[j][0] != fmt.tree_path(j)) return -(int)(200 + j);
                if (misses(lv[j], s, tp & (((size_t)1 << lg) - 1), lp[j][0], lpl[j][0], roots[j])) return -(int)(300 + j);
                continue;
            }
            for (uint32_t t = 0; t < s; ++t) if (lpl[j][t] != fmt.tree_path(j)) return -(int)(200 + j);
            for (uint32_t t = 0; t < s; ++t)
                if (misses(&lv[j][t], 1, coset_leaf(tp, lg, steps, t), lp[j][t], lpl[j][t], roots[j])) return t == 0 ? -(int)(300 + j) : -(int)(400 + j);
        }
    }
    if (left != 0) return -8;
    return 0;
}
inline int verify_proof(const uint8_t* data, size_t len, const ProofFormat& fmt, uint32_t public_last, int hash) {
    return fmt.lb ? -1 : verify_proof(data, len, fmt, &public_last, hash);   // one statement
}

// verify_proof for ext = 1 (the format above, "ext"): one statement, the same walk and the same check numbers, values of cp and of the FRI
// layers in E.  Words are reduced % P before arithmetic and compared unreduced, as there; two values of E differ when either component does.
inline int verify_proof_ext(const uint8_t* data, size_t len, const ProofFormat& fmt, uint32_t public_last, int hash) {
    if (!fmt.ok() || fmt.ext != 1 || hash == ZK_HASH_BLAKE2S || len != fmt.data_len()) return -1;
    const bool coset = fmt.coset;
    const size_t n = (size_t)1 << fmt.log_n, B = (size_t)1 << fmt.log_b, N = n << fmt.log_b;
    const uint32_t L = fmt.L(), G = fmt.groups();
    const uint8_t* p = data;
    size_t left = len;
    bool bad = false;
    auto take = [&](size_t k) -> const uint8_t* {
        if (left < k) { bad = true; return nullptr; }
        const uint8_t* r = p; p += k; left -= k; return r;
    };
    auto le32 = [](const uint8_t* r) { return (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24); };
    auto take32 = [&]() -> uint32_t { const uint8_t* r = take(4); return r ? le32(r) : 0; };
    auto take_path = [&](size_t& plen) -> const uint8_t* {
        const uint8_t* r = take(8);
        if (!r) return nullptr;
        uint64_t c = 0;
        for (int i = 0; i < 8; ++i) c |= (uint64_t)r[i] << (8 * i);
        if (c > 64) { bad = true; return nullptr; }
        plen = (size_t)c;
        return take(32 * plen);
    };
    const uint8_t *f_root = nullptr, *alphas = nullptr, *final_term = nullptr, *raws = nullptr, *roots[41] = {nullptr}, *betas[40];
    fmt.for_each_head([&](ProofFormat::Head what, uint32_t j, size_t bytes) {
        const uint8_t* r = take(bytes);
        switch (what) {
            case ProofFormat::kFTree: f_root = r; break;
            case ProofFormat::kAlphas: alphas = r; break;      // alpha0.c0, alpha0.c1, alpha1.c0, ..
            case ProofFormat::kTree: roots[j] = r; break;
            case ProofFormat::kBeta: betas[j] = r; break;      // c0, c1
            case ProofFormat::kFinal: final_term = r; break;   // c0, c1 of the free term, or the coefficients plane by plane
            case ProofFormat::kNonce: break;
            case ProofFormat::kRaws: raws = r; break;
        }
        return true;
    });
    if (bad) return -1;
    const uint32_t g = root_of_unity(fmt.log_n), h = root_of_unity(L);
    for (uint32_t qk = 0; qk < fmt.q; ++qk) {
        uint32_t fv[3], cpw[2] = {0, 0}; const uint8_t* fp[4]; size_t fpl[4] = {0, 0, 0, 0};
        uint32_t lw[40][16]; const uint8_t* lp[40][8]; size_t lpl[40][8];   // group j's words as sent: s component-0 words, then s component-1 words
        uint32_t i = 0;
        const uint32_t nf = coset ? 3 : 4;
        fmt.for_each_tuple([&](size_t s, size_t, bool one_leaf, uint32_t words) {
            uint32_t* v = i < 3 ? &fv[i] : i < nf ? cpw : lw[i - nf];
            const uint8_t** path = i < nf ? &fp[i] : lp[i - nf];
            size_t* plen = i < nf ? &fpl[i] : lpl[i - nf];
            for (size_t t = 0; t < s * words; ++t) v[t] = take32();
            for (size_t t = 0; t < (one_leaf ? 1 : s); ++t) { plen[t] = 0; path[t] = take_path(plen[t]); }
            ++i;
        });
        if (bad) return -1;
        const size_t tp = (size_t)le32(raws + 4 * qk) % (N - 2 * B);
        // value t of group j, unreduced: as sent, or slot (rot + t) % s of the group's leaf
        auto group_val = [&](uint32_t j, uint32_t t) -> Ext {
            const uint32_t steps = fmt.steps(j), s = 1u << steps;
            if (!coset) return Ext{lw[j][t], lw[j][s + t]};
            const uint32_t lg = L - fmt.round0(j);
            const size_t rot = (tp & (((size_t)1 << lg) - 1)) >> (lg - steps);
            const uint32_t u = (uint32_t)(rot + t) & (s - 1u);
            return Ext{lw[j][u], lw[j][s + u]};
        };
        if (coset) { const Ext c = group_val(0, 0); cpw[0] = c.c0; cpw[1] = c.c1; }
        const uint32_t x = mulmod(GEN_W, powmod(h, tp));
        {   // proof.rs:63-77 with the alphas in E: component j of cp takes the component-j alphas
            const uint32_t gm1 = invmod(g), gm2 = mulmod(gm1, gm1), gm3 = mulmod(gm2, gm1);
            const uint32_t i0 = invmod(sub(x, 1)), i1 = invmod(sub(x, gm2));
            const uint32_t den = mulmod(sub(powmod(x, n), 1), invmod(mulmod(mulmod(sub(x, gm3), sub(x, gm2)), sub(x, gm1))));
            const uint32_t i2 = invmod(den);
            const uint32_t f_x = fv[0] % P, f_gx = fv[1] % P, f_ggx = fv[2] % P;
            const uint32_t p0 = mulmod(sub(f_x, 1), i0), p1 = mulmod(sub(f_x, public_last % P), i1);
            const uint32_t p2 = mulmod(sub(sub(f_ggx, mulmod(f_gx, f_gx)), mulmod(f_x, f_x)), i2);
            for (uint32_t c = 0; c < 2; ++c) {
                const uint8_t* al = alphas + 4 * c;
                const uint32_t cp0 = add(add(mulmod(le32(al) % P, p0), mulmod(le32(al + 8) % P, p1)), mulmod(le32(al + 16) % P, p2));
                if (cp0 != cpw[c]) return -2;
            }
        }
        uint8_t root[32];
        auto misses = [&](const uint32_t* words, size_t count, size_t idx, const uint8_t* path, size_t plen, const uint8_t* entries) -> bool {
            compute_root_from_coset(words, count, idx & (((size_t)1 << plen) - 1), path, plen, root, hash);
            return memcmp(root, entries + 32 * (idx >> plen), 32) != 0;
        };
        for (uint32_t k = 0; k < 3; ++k) if (fpl[k] != fmt.f_path()) return -3;
        if (!coset && fpl[3] != fmt.tree_path(0)) return -3;
        if (misses(&fv[0], 1, tp, fp[0], fpl[0], f_root)) return -4;
        if (misses(&fv[1], 1, tp + B, fp[1], fpl[1], f_root)) return -5;
        if (misses(&fv[2], 1, tp + 2 * B, fp[2], fpl[2], f_root)) return -6;
        if (!coset && misses(cpw, 2, tp, fp[3], fpl[3], roots[0])) return -7;      // the leaf of one value of E: its two words
        const uint32_t inv2 = invmod(2);
        for (uint32_t j = 0; j < G; ++j) {
            const uint32_t r0 = fmt.round0(j), steps = fmt.steps(j);
            uint32_t cnt = 1u << steps;
            Ext v[8];
            for (uint32_t t = 0; t < cnt; ++t) { const Ext w = group_val(j, t); v[t] = ext_reduce(w.c0, w.c1); }
            uint32_t xk = powmod(x, (uint64_t)1 << r0);
            uint32_t om = powmod(h, (uint64_t)N >> steps);
            Ext bk = ext_reduce(le32(betas[j]), le32(betas[j] + 4));
            for (uint32_t k = 0; k < steps; ++k) {
                cnt >>= 1;
                uint32_t pt = xk;
                for (uint32_t t = 0; t < cnt; ++t) {
                    const uint32_t i2x = invmod(mulmod(pt, 2));
                    const Ext sum = ext_add(v[t], v[t + cnt]), dif = ext_sub(v[t], v[t + cnt]);
                    const Ext gx{mulmod(sum.c0, inv2), mulmod(sum.c1, inv2)}, hx{mulmod(dif.c0, i2x), mulmod(dif.c1, i2x)};
                    v[t] = ext_add(gx, ext_mul(bk, hx));
                    pt = mulmod(pt, om);
                }
                xk = mulmod(xk, xk); om = mulmod(om, om); bk = ext_mul(bk, bk);
            }
            Ext expect;
            if (j + 1 < G) expect = group_val(j + 1, 0);
            else if (!fmt.stop) expect = Ext{le32(final_term), le32(final_term + 4)};
            else {                                                               // Horner over the coefficients of E at the base-field point x^(2^R')
                const uint32_t xs = powmod(x, (uint64_t)1 << fmt.rounds());
                const size_t nc = (size_t)1 << fmt.stop;
                expect = Ext{0u, 0u};
                for (size_t k = nc; k-- > 0; )
                    expect = Ext{add(mulmod(expect.c0, xs), le32(final_term + 4 * k) % P), add(mulmod(expect.c1, xs), le32(final_term + 4 * (nc + k)) % P)};
            }
            if (!ext_eq(v[0], expect)) return -(int)(100 + j);
        }
        for (uint32_t j = 0; j < G; ++j) {
            const uint32_t lg = fmt.tree_log(j), steps = fmt.steps(j), s = 1u << steps;
            if (coset) {
                if (lpl[j][0] != fmt.tree_path(j)) return -(int)(200 + j);
                if (misses(lw[j], 2 * s, tp & (((size_t)1 << lg) - 1), lp[j][0], lpl[j][0], roots[j])) return -(int)(300 + j);   // the leaf's own message
                continue;
            }
            for (uint32_t t = 0; t < s; ++t) if (lpl[j][t] != fmt.tree_path(j)) return -(int)(200 + j);
            for (uint32_t t = 0; t < s; ++t) {
                const uint32_t pair[2] = {lw[j][t], lw[j][s + t]};
                if (misses(pair, 2, coset_leaf(tp, lg, steps, t), lp[j][t], lpl[j][t], roots[j])) return t == 0 ? -(int)(300 + j) : -(int)(400 + j);
            }
        }
    }
    if (left != 0) return -8;
    return 0;
}

// the reference verifier reads the challenges out of the proof
// (proof.rs:22-37) and never checks Proof.state (proof.rs:6); the author flags this as unfinished
// (readme.md:1).  This replays the Fiat-Shamir channel over the proof bytes in the prover's commit
// order (prover.rs:85, :163-165, :180, :200, :224, :254, :263, :274-277, :288: one commit per tuple; coset: three f tuples and one
// tuple per group), checks that every
// challenge equals the one the transcript yields at that point and that the final state matches.  There are 3 + G + q challenges.
// Returns 0, or -(1000 + k) for the k-th challenge / -1998 for a grinding nonce whose hash has fewer than `grind` leading zero
// bits (checked after the betas and before the first query challenge; it does not advance k) / -1999 for the state.
// stop > 0: 3 + G' + q challenges; the coefficients are one commit, in the place of the last root and the free term.
// cap > 0: every root commit is one commit of the tree's 2^ce digests, and a tuple's paths are ce digests shorter.
// lb > 0: 3 * 2^lb + G + q challenges; the f level is one commit, each of the 3 * 2^lb f tuples of a query one commit.
// rows: the same challenges; the f cap is one commit, each of the three row tuples of a query one commit.
inline int verify_transcript(const uint8_t* data, size_t len, const uint8_t state[32], const ProofFormat& fmt) {
    if (!fmt.ok() || len != fmt.data_len()) return -1;
    Channel ch;
    const uint8_t* p = data;
    int k = 0, rc = 0;
    auto commit = [&](size_t n) { ch.commit_bytes(p, n); p += n; };
    auto challenge = [&]() -> bool {
        uint32_t expect = ((uint32_t)ch.state[0] << 24) | ((uint32_t)ch.state[1] << 16) | ((uint32_t)ch.state[2] << 8) | ch.state[3];
        uint32_t got = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        ++k;
        if (got != expect) return false;
        commit(4);
        return true;
    };
    fmt.for_each_head([&](ProofFormat::Head what, uint32_t, size_t bytes) {
        if (what == ProofFormat::kAlphas || what == ProofFormat::kBeta || what == ProofFormat::kRaws) {
            for (size_t i = 0; i < bytes; i += 4) if (!challenge()) { rc = -(1000 + k); return false; }
            return true;
        }
        commit(bytes);                                      // a root (cap: its 2^ce digests), the free term or the coefficients, the nonce
        if (what == ProofFormat::kNonce) {                  // the commit is SHA-256(S || le64(w))
            const uint32_t w0 = ((uint32_t)ch.state[0] << 24) | ((uint32_t)ch.state[1] << 16) | ((uint32_t)ch.state[2] << 8) | ch.state[3];
            if (!grind_word_ok(w0, fmt.grind)) { rc = -1998; return false; }
        }
        return true;
    });
    if (rc) return rc;
    for (uint32_t j = 0; j < fmt.q; ++j) fmt.for_each_tuple([&](size_t s, size_t plen, bool one_leaf, uint32_t words) { commit(ProofFormat::tuple_bytes(s, plen, one_leaf, words)); });
    if (memcmp(ch.state, state, 32)) return -1999;
    return 0;
}

}  // namespace zk
