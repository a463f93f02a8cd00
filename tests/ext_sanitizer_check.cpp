// The host-only verifier of the ext = 1 format (transcript.hpp, ProofFormat::ext, verify_proof_ext) and the arithmetic of E (ext.hpp) under
// ASan + UBSan: the arithmetic against its own laws, the format against itself, then a model proof (tests/ext_ref.py) valid, truncated,
// bit-flipped, with huge path counts in a cp or group tuple, read as the other ext_log, and random bytes.
// Built and run by tests/test_host_sanitizers_ext.py (CPU only).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../zkstark_amd/csrc/transcript.hpp"

using namespace zk;

static uint32_t rng_state = 24680;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static Ext rnd_ext() { return Ext{(uint32_t)(((uint64_t)rnd() << 8 | (rnd() & 255u)) % P), (uint32_t)(((uint64_t)rnd() << 8 | (rnd() & 255u)) % P)}; }

static int field_self_check() {
    const Ext one{1u, 0u}, u{0u, 1u};
    if (!ext_eq(ext_mul(u, u), Ext{EXT_NONRESIDUE, 0u}) || powmod(EXT_NONRESIDUE, (P - 1) / 2) != P - 1) { printf("u^2 is not the non-residue\n"); return 1; }
    const Ext edge[] = {Ext{0u, 0u}, Ext{P - 1, P - 1}, u, one, Ext{P - 1, 0u}, Ext{0u, P - 1}};
    for (int k = 0; k < 2000; ++k) {
        const Ext a = k < 6 ? edge[k] : rnd_ext(), b = k % 7 == 0 ? edge[k % 6] : rnd_ext(), c = rnd_ext();
        if (a.c0 >= P || a.c1 >= P) return 1;
        if (!ext_eq(ext_mul(a, b), ext_mul(b, a)) || !ext_eq(ext_mul(ext_mul(a, b), c), ext_mul(a, ext_mul(b, c))) ||
            !ext_eq(ext_mul(a, ext_add(b, c)), ext_add(ext_mul(a, b), ext_mul(a, c))) || !ext_eq(ext_sub(ext_add(a, b), b), a)) {
            printf("ring laws fail at (%u, %u)\n", a.c0, a.c1);
            return 1;
        }
        if (!ext_is_zero(a) && (!ext_eq(ext_mul(a, ext_inv(a)), one) || !ext_eq(ext_pow(a, (uint64_t)P * P - 1), one))) { printf("inverse fails at (%u, %u)\n", a.c0, a.c1); return 1; }
        if (!ext_eq(ext_pow(a, 5), ext_mul(ext_mul(ext_mul(a, a), ext_mul(a, a)), a))) { printf("pow fails\n"); return 1; }
    }
    printf("field self-check: ok\n");
    return 0;
}

// the length is the sum of the two walks, the tuples of the walk carry what for_each_opening fetches (2^ext words per value of a layer >= 1), and
// ext = 0 leaves every length as it was
static int format_self_check() {
    size_t formats = 0;
    for (uint32_t log_n : {2u, 5u, 10u}) for (uint32_t log_b : {1u, 3u}) for (uint32_t fold = 1; fold <= 3; ++fold) for (int coset = 0; coset < 2; ++coset)
    for (uint32_t stop : {0u, 1u, 4u}) for (uint32_t cap : {0u, 3u, 8u}) for (uint32_t q : {1u, 3u}) for (uint32_t grind : {0u, 8u}) {
        if (!stop_ok(log_n, log_b, stop)) continue;
        const ProofFormat base{.log_n = log_n, .log_b = log_b, .q = q, .grind = grind, .fold = fold, .coset = coset != 0, .stop = stop, .cap = cap};
        ProofFormat f = base;
        f.ext = 1;
        ProofFormat two = f, shared = f;
        two.ext = 2; shared.lb = 1;
        if (!f.ok() || two.ok() || shared.ok()) { printf("ok() wrong for ext\n"); return 1; }
        size_t words = 0, owords = 0, digs = 0, odigs = 0, base_words = 0;
        f.for_each_tuple([&](size_t s, size_t plen, bool one_leaf, uint32_t w) { words += s * w; digs += (one_leaf ? 1 : s) * plen; });
        base.for_each_tuple([&](size_t s, size_t, bool) { base_words += s; });
        f.for_each_opening(1, [&](uint32_t layer, uint32_t log_leaves, size_t, uint32_t slots_log) {
            owords += ((size_t)1 << slots_log) << (layer ? 1 : 0); odigs += log_leaves - cap_eff(cap, log_leaves);
        });
        const size_t G = f.groups();
        const size_t want = base.data_len() + 12 + 4 * G + ((size_t)4 << stop) + q * 4 * (base_words - 3);
        if (f.data_len() != want || words != owords || digs != odigs || words != 2 * base_words - 3) {
            printf("format inconsistent: %u %u %u %u %d %u %u: len %zu want %zu, words %zu / %zu, digests %zu / %zu\n", log_n, log_b, q, fold, coset, stop, cap,
                   f.data_len(), want, words, owords, digs, odigs);
            return 1;
        }
        ++formats;
    }
    printf("format self-check: %zu formats\n", formats);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 13) { fprintf(stderr, "usage: check proof.bin public_last log_n log_b hash q grind fold coset stop cap state-hex\n"); return 2; }
    if (field_self_check() || format_self_check()) return 1;
    std::vector<uint8_t> proof(1 << 22);
    FILE* fh = fopen(argv[1], "rb");
    proof.resize(fh ? fread(proof.data(), 1, proof.size(), fh) : 0);
    if (fh) fclose(fh);
    const uint32_t public_last = (uint32_t)strtoul(argv[2], nullptr, 10);
    ProofFormat fmt{.log_n = (uint32_t)atoi(argv[3]), .log_b = (uint32_t)atoi(argv[4])};
    const int hash = atoi(argv[5]);
    fmt.q = atoi(argv[6]); fmt.grind = atoi(argv[7]); fmt.fold = atoi(argv[8]); fmt.coset = atoi(argv[9]) != 0; fmt.stop = atoi(argv[10]); fmt.cap = atoi(argv[11]);
    fmt.ext = 1;
    if (proof.empty() || strlen(argv[12]) != 64) return 2;
    uint8_t state[32];
    for (int i = 0; i < 32; ++i) { unsigned b = 0; sscanf(argv[12] + 2 * i, "%2x", &b); state[i] = (uint8_t)b; }
    // every input is copied into a heap buffer of exactly its length, so a read past it is a heap overflow the sanitizer reports
    auto check = [&](const uint8_t* data, size_t len, const ProofFormat& as, bool strict, int kind) {
        std::vector<uint8_t> exact(data, data + len);
        const int rc = strict ? verify_transcript(exact.data(), len, state, as) : 0;
        return rc ? rc : verify_proof(exact.data(), len, as, public_last, kind);
    };
    for (bool strict : {false, true}) {
        const int ok = check(proof.data(), proof.size(), fmt, strict, hash);
        if (ok != 0) { printf("valid proof rejected: %d (strict %d)\n", ok, (int)strict); return 1; }
    }
    if (check(proof.data(), proof.size(), fmt, false, ZK_HASH_BLAKE2S) != -1) { printf("BLAKE2s with ext was not refused\n"); return 1; }
    int rejected = 0, total = 0;
    for (size_t cut = 0; cut < proof.size(); cut += 1 + proof.size() / 61)
        for (bool strict : {false, true}) { ++total; rejected += check(proof.data(), cut, fmt, strict, hash) == -1; }
    for (int k = 0; k < 400; ++k) {                                                    // bit flips: the replay sees every byte
        std::vector<uint8_t> bad = proof;
        bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() % 8));
        ++total; rejected += check(bad.data(), bad.size(), fmt, true, hash) != 0;
        (void)check(bad.data(), bad.size(), fmt, false, hash);
    }
    // huge and off-by-a-few path counts: the count of every tuple of the first query in turn
    size_t head = 0;
    fmt.for_each_head([&](ProofFormat::Head, uint32_t, size_t n) { head += n; return true; });
    std::vector<size_t> counts;
    size_t at = head;
    fmt.for_each_tuple([&](size_t s, size_t plen, bool one_leaf, uint32_t words) {
        counts.push_back(at + 4 * s * words);
        at += ProofFormat::tuple_bytes(s, plen, one_leaf, words);
    });
    for (size_t k = 0; k < 4 * counts.size(); ++k) {
        std::vector<uint8_t> bad = proof;
        const size_t c = counts[k % counts.size()];
        if (k & 1) bad[c] = (uint8_t)(bad[c] + 1 + rnd() % 3);
        else for (int i = 0; i < 8; ++i) bad[c + i] = (uint8_t)rnd();
        ++total; rejected += check(bad.data(), bad.size(), fmt, false, hash) != 0;
    }
    {   // the same bytes read as the other ext_log, and a format the verifier does not take
        ProofFormat other = fmt;
        other.ext = 0;
        for (bool strict : {false, true}) {                                             // (a plain format without cap or stop has no length check: any number)
            const int rc = check(proof.data(), proof.size(), other, strict, hash);
            ++total; rejected += (other.stop || other.cap || strict) ? rc == -1 : rc != 0;
        }
        other.ext = 2;
        for (bool strict : {false, true}) { ++total; rejected += check(proof.data(), proof.size(), other, strict, hash) == -1; }
    }
    for (int k = 0; k < 100; ++k) {                                                    // random bytes of the right and of wrong sizes
        std::vector<uint8_t> junk(k % 4 == 0 ? fmt.data_len() : rnd() % (2 * proof.size() + 1));
        for (auto& b : junk) b = (uint8_t)rnd();
        for (bool strict : {false, true}) { ++total; rejected += check(junk.data(), junk.size(), fmt, strict, hash) != 0; }
    }
    printf("ok: valid accepted, %d of %d malformed inputs rejected\n", rejected, total);
    return rejected == total ? 0 : 1;
}
