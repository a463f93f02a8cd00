// Host-only code of the product (transcript, verifier, field-native hash) under ASan + UBSan:
// the verifier parses untrusted bytes, so it is fed valid, truncated, bit-flipped and random inputs.
// Built and run by tests/test_host_sanitizers.py (CPU only; GPU sanitizers are not available).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../zkstark_amd/csrc/transcript.hpp"

using namespace zk;

static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// ProofFormat against itself over the admissible grid: the length is the sum of its two walks, and the openings the provers fetch
// (for_each_opening) are the values and digests the tuples they commit (for_each_tuple) carry.
static int format_self_check() {
    size_t formats = 0;
    for (uint32_t log_n = 2; log_n <= 12; ++log_n) for (uint32_t log_b = 1; log_b <= 5; ++log_b) for (uint32_t fold = 1; fold <= 3; ++fold)
    for (int coset = 0; coset < 2; ++coset) for (uint32_t stop = 0; stop <= 9; ++stop) for (uint32_t cap = 0; cap <= 8; ++cap)
    for (uint32_t q : {1u, 3u}) for (uint32_t grind : {0u, 4u}) {
        if (!stop_ok(log_n, log_b, stop)) continue;
        const ProofFormat f{.log_n = log_n, .log_b = log_b, .q = q, .grind = grind, .fold = fold, .coset = coset != 0, .stop = stop, .cap = cap};
        if (!f.ok()) { printf("format refused: %u %u %u %u %u %d %u %u\n", log_n, log_b, q, grind, fold, coset, stop, cap); return 1; }
        size_t head = 0, bytes = 0, tvals = 0, tdigs = 0, ovals = 0, odigs = 0;
        f.for_each_head([&](ProofFormat::Head, uint32_t, size_t n) { head += n; return true; });
        f.for_each_tuple([&](size_t s, size_t plen, bool one_leaf) {
            bytes += Channel::group_bytes(s, plen, one_leaf); tvals += s; tdigs += (one_leaf ? 1 : s) * plen;
        });
        f.for_each_opening(5, [&](uint32_t, uint32_t log_leaves, size_t, uint32_t slots_log) {
            ovals += (size_t)1 << slots_log; odigs += log_leaves - cap_eff(cap, log_leaves);
        });
        if (f.data_len() != head + q * bytes || tvals != ovals || tdigs != odigs) {
            printf("format inconsistent: %u %u %u %u %u %d %u %u: len %zu, walks %zu + %u * %zu, values %zu / %zu, digests %zu / %zu\n", log_n, log_b, q,
                   grind, fold, coset, stop, cap, f.data_len(), head, q, bytes, tvals, ovals, tdigs, odigs);
            return 1;
        }
        ++formats;
    }
    printf("format self-check: %zu formats\n", formats);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 6 && argc != 13) { fprintf(stderr, "usage: check proof.bin log_n log_b public_last hash [q grind fold coset stop cap state-hex]\n"); return 2; }
    if (format_self_check()) return 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> proof(1 << 20);
    proof.resize(fread(proof.data(), 1, proof.size(), f));
    fclose(f);
    uint32_t log_n = atoi(argv[2]), log_b = atoi(argv[3]), last = strtoul(argv[4], nullptr, 10);
    int hash = atoi(argv[5]);
    ProofFormat fmt{.log_n = log_n, .log_b = log_b};
    uint8_t given[32];
    const uint8_t* state = nullptr;                                                    // given: the replay runs first (the strict verifier)
    if (argc == 13) {
        fmt.q = atoi(argv[6]); fmt.grind = atoi(argv[7]); fmt.fold = atoi(argv[8]); fmt.coset = atoi(argv[9]) != 0; fmt.stop = atoi(argv[10]); fmt.cap = atoi(argv[11]);
        if (strlen(argv[12]) != 64) return 2;
        for (int i = 0; i < 32; ++i) { unsigned b = 0; sscanf(argv[12] + 2 * i, "%2x", &b); given[i] = (uint8_t)b; }
        state = given;
    }
    auto check = [&](const uint8_t* data, size_t len, ProofFormat as) {
        const int rc = state ? verify_transcript(data, len, state, as) : 0;
        return rc ? rc : verify_proof(data, len, as, last, hash);
    };
    int ok = check(proof.data(), proof.size(), fmt);
    if (ok != 0) { printf("valid proof rejected: %d\n", ok); return 1; }
    // The reference verifier never uses the root of the LAST FRI layer (proof.rs:129-148 opens layers
    // 0..R-1 only; the free term stands for layer R), so flips inside those 32 bytes are accepted by
    // zk_verify exactly as by the reference; zk_verify_strict catches them through the transcript.
    // A stopped proof has no such root; the strict verifier checks every byte.
    size_t last_root = 0, last_root_len = 0, head = 0;
    fmt.for_each_head([&](ProofFormat::Head what, uint32_t j, size_t n) {
        if (what == ProofFormat::kTree && j == fmt.groups()) { last_root = head; last_root_len = n; }
        head += n;
        return true;
    });
    const size_t first_plen = head + 4;                                                // first path length field: behind the first f value
    if (argc == 6 && (last_root != 32 + 12 + 32 + (size_t)(log_n - 1) * 36 + 4 || last_root_len != 32 || first_plen != 32 + 12 + 32 + (size_t)log_n * 36 + 8 + 4)) {
        printf("the header walk of the default format puts the last root at %zu and the first path length at %zu\n", last_root, first_plen);
        return 1;
    }
    if (state) last_root_len = 0;
    int rejected = 0, total = 0;
    for (size_t cut = 0; cut < proof.size(); cut += 1 + proof.size() / 97) {          // truncations
        ++total; rejected += check(proof.data(), cut, fmt) != 0;
    }
    for (int k = 0; k < 300; ++k) {                                                    // bit flips
        std::vector<uint8_t> bad = proof;
        size_t pos = rnd() % bad.size();
        if (pos >= last_root && pos < last_root + last_root_len) pos = (pos + 64) % bad.size();
        bad[pos] ^= (uint8_t)(1u << (rnd() % 8));
        ++total; rejected += check(bad.data(), bad.size(), fmt) != 0;
    }
    for (int k = 0; k < 100; ++k) {                                                    // random bytes, wrong sizes
        std::vector<uint8_t> junk(rnd() % (2 * proof.size() + 1));
        for (auto& b : junk) b = (uint8_t)rnd();
        ProofFormat other = fmt;
        other.log_n += k % 3;
        ++total; rejected += check(junk.data(), junk.size(), other) != 0;
    }
    for (int k = 0; k < 50; ++k) {                                                     // huge path counts
        std::vector<uint8_t> bad = proof;
        for (int i = 0; i < 8; ++i) bad[first_plen + i] = (uint8_t)rnd();
        ++total; rejected += check(bad.data(), bad.size(), fmt) != 0;
    }
    uint8_t st[32] = {0};
    (void)verify_transcript(proof.data(), proof.size(), st, fmt);                      // wrong state: must not crash
    (void)verify_transcript(proof.data(), proof.size() / 2, st, fmt);
    Channel ch;                                                                        // channel.rs
    ch.commit_hash(st);
    (void)ch.get_u32();
    uint8_t path[3 * 32] = {0}, out[32];
    ch.commit_val_path(7, path, 3);
    ch.commit_pair_paths(1, 2, path, path, 3);
    compute_root_from_path(5, 3, path, 3, out, 0);
    compute_root_from_path(5, 3, path, 3, out, 1);
    if (last_root_len) {   // the unchecked last root: lax verifier accepts, transcript replay rejects
        std::vector<uint8_t> bad = proof;
        bad[last_root + 5] ^= 1;
        if (verify_proof(bad.data(), bad.size(), fmt, last, hash) != 0) { printf("last-root flip rejected by the lax verifier?\n"); return 1; }
    }
    printf("ok: valid accepted, %d of %d malformed inputs rejected\n", rejected, total);
    return rejected == total ? 0 : 1;
}
