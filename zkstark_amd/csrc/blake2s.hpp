// blake2s.hpp -- BLAKE2s-256 (RFC 7693) as a Merkle hash (ZK_HASH_BLAKE2S), host and device from one definition.
//
// Unkeyed, 32-byte digest, no salt, no personalisation: h = IV, h[0] ^= 0x01010020.  Both shapes of the tree are ONE compression
// with the last-block flag:
//   leaf : the s <= 8 slots, 4 bytes big-endian each (the message the SHA-256 leaf hashes), t = 4 s; the other message words are zero
//          and fold away
//   inner: left || right, t = 64
// There is no message schedule: round r reads the sixteen message words through the fixed permutation SIGMA[r % 10], folded at compile
// time (the rounds are template instances), so the words stay registers with constant indices.
//
// Byte order, decided HERE and nowhere else: a Digest holds a digest as eight words read BIG-endian from its 32 bytes, for every hash
// (sha256.hpp: digest_words_to_bytes; what the heap, the mailbox, paths and proofs carry).  BLAKE2s words are little-endian, so this
// file swaps at its boundary: the message words of an inner node are the byte-swapped words of the two child Digests, a leaf's message
// word is the byte-swapped slot (big-endian bytes read as a little-endian word), and the eight output words are swapped into the
// Digest.  24 byte permutes per inner node (one instruction each) against ~1 000 for the compression; everything outside this file
// is hash-agnostic and the bytes that leave the library are hashlib.blake2s(msg).digest().
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sha256.hpp"

namespace zk {

// the IV is SHA-256's (SHA_IV)
constexpr uint32_t kB2sParam0 = 0x01010020u;   // digest length 32, key length 0, fanout 1, depth 1
constexpr uint8_t B2S_SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

ZK_SHA_HD uint32_t b2s_bswap(uint32_t x) { return __builtin_bswap32(x); }

// G: 4 additions with a message word folded into two of them, 4 xors, 4 rotations (16, 12, 8, 7)
ZK_SHA_HD void b2s_g(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t x, uint32_t y) {
    a = a + b + x; d = sha_rotr(d ^ a, 16);
    c = c + d;     b = sha_rotr(b ^ c, 12);
    a = a + b + y; d = sha_rotr(d ^ a, 8);
    c = c + d;     b = sha_rotr(b ^ c, 7);
}
template <int R>
ZK_SHA_HD void b2s_round(uint32_t (&v)[16], const uint32_t (&m)[16]) {
    b2s_g(v[0], v[4], v[8], v[12], m[B2S_SIGMA[R][0]], m[B2S_SIGMA[R][1]]);
    b2s_g(v[1], v[5], v[9], v[13], m[B2S_SIGMA[R][2]], m[B2S_SIGMA[R][3]]);
    b2s_g(v[2], v[6], v[10], v[14], m[B2S_SIGMA[R][4]], m[B2S_SIGMA[R][5]]);
    b2s_g(v[3], v[7], v[11], v[15], m[B2S_SIGMA[R][6]], m[B2S_SIGMA[R][7]]);
    b2s_g(v[0], v[5], v[10], v[15], m[B2S_SIGMA[R][8]], m[B2S_SIGMA[R][9]]);
    b2s_g(v[1], v[6], v[11], v[12], m[B2S_SIGMA[R][10]], m[B2S_SIGMA[R][11]]);
    b2s_g(v[2], v[7], v[8], v[13], m[B2S_SIGMA[R][12]], m[B2S_SIGMA[R][13]]);
    b2s_g(v[3], v[4], v[9], v[14], m[B2S_SIGMA[R][14]], m[B2S_SIGMA[R][15]]);
}

// The whole hash of a message of t <= 64 bytes that lies in m as little-endian words (zero beyond the message): one compression from
// the parameter block's state, counter t, last-block flag.  Every call site is inlined, so constant message words fold away.
ZK_SHA_HD Digest blake2s_single(const uint32_t (&m)[16], uint32_t t) {
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = SHA_IV[i]; v[8 + i] = SHA_IV[i]; }
    v[0] ^= kB2sParam0;
    v[12] ^= t;                    // t0; t1 = 0
    v[14] = ~v[14];                // f0 = 0xffffffff: the last block
    b2s_round<0>(v, m); b2s_round<1>(v, m); b2s_round<2>(v, m); b2s_round<3>(v, m); b2s_round<4>(v, m);
    b2s_round<5>(v, m); b2s_round<6>(v, m); b2s_round<7>(v, m); b2s_round<8>(v, m); b2s_round<9>(v, m);
    Digest d;
#pragma unroll
    for (int i = 0; i < 8; ++i) d.w[i] = b2s_bswap((SHA_IV[i] ^ (i == 0 ? kB2sParam0 : 0u)) ^ v[i] ^ v[8 + i]);
    return d;
}

// BLAKE2s-256(left || right)
ZK_SHA_HD Digest blake2s_inner(const Digest& l, const Digest& r) {
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) { m[i] = b2s_bswap(l.w[i]); m[8 + i] = b2s_bswap(r.w[i]); }
    return blake2s_single(m, 64u);
}
// BLAKE2s-256 of S <= 8 slots, 4 bytes big-endian each; S = 1 is the one-value leaf
template <int S>
ZK_SHA_HD Digest blake2s_slots(const uint32_t (&v)[S]) {
    static_assert(S >= 1 && S <= 8, "a leaf holds at most eight slots");
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = i < S ? b2s_bswap(v[i]) : 0u;
    return blake2s_single(m, 4u * S);
}
ZK_SHA_HD Digest blake2s_leaf(uint32_t value) {
    const uint32_t v[1] = {value};
    return blake2s_slots<1>(v);
}
// the same with the slot count known only at run time (host: the verifier's leaves); s <= 8
inline Digest blake2s_coset_leaf(const uint32_t* slots, size_t s) {
    uint32_t m[16] = {0};
    for (size_t i = 0; i < s && i < 8; ++i) m[i] = b2s_bswap(slots[i]);
    return blake2s_single(m, (uint32_t)(4 * s));
}

}  // namespace zk
