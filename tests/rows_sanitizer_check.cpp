// The row-leaf side of the host-only verifier (transcript.hpp with ProofFormat::rows) and the row leaf hash under ASan + UBSan: the format
// against itself for every width, the leaf hash at every width from buffers of exactly m values, then a model proof (tests/rows_ref.py)
// valid, truncated, bit-flipped, with huge path counts in a row tuple, read without row leaves and as another width, and random bytes.
// Built and run by tests/test_host_sanitizers_rows.py (CPU only).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../zkstark_amd/csrc/transcript.hpp"

using namespace zk;

static uint32_t rng_state = 97531;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// the length is the sum of the two walks and is the single proof's plus 12 (M - 1) (1 + q); what the prover fetches (for_each_opening, at
// x = 1 < N - 2B) is what the tuples carry: three leaves of layer 0, each of 2^lb slots, at 1, 1 + B, 1 + 2B
static int format_self_check() {
    size_t formats = 0;
    for (uint32_t log_n : {2u, 5u, 10u}) for (uint32_t log_b : {1u, 3u}) for (uint32_t fold = 1; fold <= 3; ++fold) for (int coset = 0; coset < 2; ++coset)
    for (uint32_t stop : {0u, 1u, 4u}) for (uint32_t cap : {0u, 3u, 8u}) for (uint32_t q : {1u, 3u}) for (uint32_t lb = 0; lb <= kMaxSharedLog + 1; ++lb) {
        if (!stop_ok(log_n, log_b, stop)) continue;
        const ProofFormat f{.log_n = log_n, .log_b = log_b, .q = q, .fold = fold, .coset = coset != 0, .stop = stop, .cap = cap, .lb = lb, .rows = true};
        if (f.ok() != (lb >= 1 && lb <= kMaxSharedLog)) { printf("ok() wrong for rows with lb %u\n", lb); return 1; }
        if (!f.ok()) continue;
        ProofFormat one = f;
        one.lb = 0; one.rows = false;
        const size_t M = (size_t)1 << lb;
        const size_t want = one.data_len() + 12 * (M - 1) * (1 + q);
        size_t tvals = 0, tdigs = 0, ovals = 0, odigs = 0, f_seen = 0, head_f = 0;
        bool order = true;
        f.for_each_head([&](ProofFormat::Head what, uint32_t, size_t n) { if (what == ProofFormat::kFTree) head_f = n; return true; });
        f.for_each_tuple([&](size_t s, size_t plen, bool one_leaf) { tvals += s; tdigs += (one_leaf ? 1 : s) * plen; });
        f.for_each_opening(1, [&](uint32_t layer, uint32_t log_leaves, size_t leaf, uint32_t slots_log) {
            ovals += (size_t)1 << slots_log; odigs += log_leaves - cap_eff(cap, log_leaves);
            if (layer == 0) { order = order && slots_log == lb && log_leaves == f.L() && leaf == 1 + (f_seen << log_b); ++f_seen; }
            else order = order && leaf < ((size_t)1 << log_leaves);
        });
        if (f.data_len() != want || tvals != ovals || tdigs != odigs || f_seen != 3 || !order || head_f != ((size_t)32 << f.f_cap())) {
            printf("format inconsistent: %u %u %u %u %d %u %u lb %u: len %zu want %zu, values %zu / %zu, digests %zu / %zu, f openings %zu\n", log_n, log_b, q, fold,
                   coset, stop, cap, lb, f.data_len(), want, tvals, ovals, tdigs, odigs, f_seen);
            return 1;
        }
        ++formats;
    }
    printf("format self-check: %zu formats\n", formats);
    return 0;
}

// every width from a heap buffer of exactly m values; M <= 8 is the coset leaf, and the SHA-256 leaf is the digest of the whole message
static int leaf_self_check() {
    for (uint32_t m = 1; m <= (1u << kMaxSharedLog); m *= 2) {
        std::vector<uint32_t> v(m);
        for (auto& x : v) x = rnd() % P;
        uint8_t a[32], b[32];
        host_coset_leaf_hash(v.data(), m, a, ZK_HASH_SHA256);
        std::vector<uint8_t> be(4 * m);
        for (uint32_t u = 0; u < m; ++u) for (int i = 0; i < 4; ++i) be[4 * u + i] = (uint8_t)(v[u] >> (24 - 8 * i));
        Sha256 h; h.update(be.data(), be.size()); h.finalize(b);
        if (memcmp(a, b, 32)) { printf("SHA-256 row leaf of %u values is not the digest of the message\n", m); return 1; }
        host_coset_leaf_hash(v.data(), m, a, ZK_HASH_FIELD);
        digest_words_to_bytes(fieldhash_row_leaf(v.data(), m, host_fieldhash_consts()).w, b);
        if (memcmp(a, b, 32)) { printf("field row leaf of %u values differs\n", m); return 1; }
        if (m <= 8) {
            digest_words_to_bytes(fieldhash_coset_leaf(v.data(), m, host_fieldhash_consts()).w, b);
            if (memcmp(a, b, 32)) { printf("field row leaf of %u values is not the coset leaf\n", m); return 1; }
        }
        compute_root_from_coset(v.data(), m, 5, nullptr, 0, b, ZK_HASH_FIELD);
        if (memcmp(a, b, 32)) { printf("a path of no digests changes the leaf\n"); return 1; }
    }
    printf("leaf self-check: widths 1 .. %u\n", 1u << kMaxSharedLog);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 14) { fprintf(stderr, "usage: check proof.bin last.bin log_n log_b lb hash q grind fold coset stop cap state-hex\n"); return 2; }
    if (format_self_check() || leaf_self_check()) return 1;
    auto slurp = [](const char* path) {
        std::vector<uint8_t> v(1 << 22);
        FILE* f = fopen(path, "rb");
        v.resize(f ? fread(v.data(), 1, v.size(), f) : 0);
        if (f) fclose(f);
        return v;
    };
    const std::vector<uint8_t> proof = slurp(argv[1]), last_bytes = slurp(argv[2]);
    ProofFormat fmt{.log_n = (uint32_t)atoi(argv[3]), .log_b = (uint32_t)atoi(argv[4])};
    fmt.lb = atoi(argv[5]);
    fmt.rows = true;
    const int hash = atoi(argv[6]);
    fmt.q = atoi(argv[7]); fmt.grind = atoi(argv[8]); fmt.fold = atoi(argv[9]); fmt.coset = atoi(argv[10]) != 0; fmt.stop = atoi(argv[11]); fmt.cap = atoi(argv[12]);
    if (proof.empty() || last_bytes.size() != ((size_t)4 << fmt.lb) || strlen(argv[13]) != 64) return 2;
    // EXACTLY 2^lb values, so a read past the statements of the format under test is a heap overflow the sanitizer reports; formats of
    // another width get a table of their own size
    std::vector<uint32_t> last((size_t)1 << fmt.lb);
    memcpy(last.data(), last_bytes.data(), last_bytes.size());
    uint8_t state[32];
    for (int i = 0; i < 32; ++i) { unsigned b = 0; sscanf(argv[13] + 2 * i, "%2x", &b); state[i] = (uint8_t)b; }
    auto check = [&](const uint8_t* data, size_t len, const ProofFormat& as, bool strict, int kind) {
        std::vector<uint32_t> mine((size_t)1 << (as.lb <= kMaxSharedLog ? as.lb : 0));
        for (size_t i = 0; i < mine.size(); ++i) mine[i] = last[i % last.size()];
        const int rc = strict ? verify_transcript(data, len, state, as) : 0;
        return rc ? rc : verify_proof(data, len, as, mine.data(), kind);
    };
    for (bool strict : {false, true}) {
        const int ok = check(proof.data(), proof.size(), fmt, strict, hash);
        if (ok != 0) { printf("valid proof rejected: %d (strict %d)\n", ok, (int)strict); return 1; }
    }
    if (check(proof.data(), proof.size(), fmt, false, ZK_HASH_BLAKE2S) != -1) { printf("BLAKE2s row leaves were not refused\n"); return 1; }
    int rejected = 0, total = 0;
    for (size_t cut = 0; cut < proof.size(); cut += 1 + proof.size() / 61)
        for (bool strict : {false, true}) { ++total; rejected += check(proof.data(), cut, fmt, strict, hash) == -1; }
    for (int k = 0; k < 400; ++k) {                                                    // bit flips: the replay sees every byte
        std::vector<uint8_t> bad = proof;
        bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() % 8));
        ++total; rejected += check(bad.data(), bad.size(), fmt, true, hash) != 0;
        (void)check(bad.data(), bad.size(), fmt, false, hash);
    }
    size_t head = 0;
    fmt.for_each_head([&](ProofFormat::Head, uint32_t, size_t n) { head += n; return true; });
    for (int k = 0; k < 60; ++k) {                                                     // huge and off-by-a-few path counts in a row tuple
        std::vector<uint8_t> bad = proof;
        const size_t at = head + (rnd() % 3u) * Channel::group_bytes((size_t)1 << fmt.lb, fmt.f_path(), true) + ((size_t)4 << fmt.lb);
        if (k & 1) bad[at] = (uint8_t)(bad[at] + 1 + rnd() % 3);
        else for (int i = 0; i < 8; ++i) bad[at + i] = (uint8_t)rnd();
        ++total; rejected += check(bad.data(), bad.size(), fmt, false, hash) != 0;
    }
    for (uint32_t lb = 0; lb <= kMaxSharedLog + 1; ++lb)                                // the same bytes without row leaves and as another width: -1
        for (bool rows : {false, true}) {
            if (lb == fmt.lb && rows) continue;
            ProofFormat other = fmt;
            other.lb = lb; other.rows = rows;
            for (bool strict : {false, true}) {                                         // (a plain format without cap or stop has no length check: any number)
                const int rc = check(proof.data(), proof.size(), other, strict, hash);
                ++total; rejected += lb == 0 && !rows && !strict ? rc != 0 : rc == -1;
            }
        }
    for (int k = 0; k < 100; ++k) {                                                    // random bytes of the right and of wrong sizes
        ProofFormat other = fmt;
        other.lb = 1 + k % kMaxSharedLog;
        std::vector<uint8_t> junk(k % 4 == 0 ? other.data_len() : rnd() % (2 * proof.size() + 1));
        for (auto& b : junk) b = (uint8_t)rnd();
        for (bool strict : {false, true}) { ++total; rejected += check(junk.data(), junk.size(), other, strict, hash) != 0; }
    }
    printf("ok: valid accepted, %d of %d malformed inputs rejected\n", rejected, total);
    return rejected == total ? 0 : 1;
}
