/*
 * zkstark_amd.h -- C ABI of the MI355X-native STARK-101 prover path.
 *
 * Drop-in boundary for the hot path of Crocodoctopus/zkstark
 * (trace -> LDE -> Merkle commit -> composition -> FRI fold -> proof).  The
 * reference is a bin-only Rust crate with no FFI; the seams below are the L0
 * functions prover.rs calls.  Each entry point cites the
 * reference interface it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the Rust `extern "C"` block and the prover.rs-shaped
 * wrapper a maintainer would add.
 *
 * Conventions
 *   - every function returns int: 0 = ZK_OK, negative = error (never aborts,
 *     never throws across the boundary; the reference panics instead);
 *     zk_last_error() gives the message of the last failure on this thread;
 *   - the caller owns all host buffers; device state lives behind zk_ctx;
 *   - one context is used from one host thread at a time;
 *   - field elements cross as uint32_t canonical residues in [0, P),
 *     P = 3221225473 (main.rs:13); raw u32 challenges >= P are accepted and
 *     reduced inside (field.rs:20-24);
 *   - digests cross as 32 raw bytes in SHA-256 byte order (merkle.rs:9 Hash);
 *   - layers and trees are addressed by id: 0 = f_eval (prover.rs:70, :81),
 *     1 + r = FRI layer r (cp_evals[r] / cp_eval_merkles[r], prover.rs:192-221),
 *     r = 0 .. log_n.
 */
#ifndef ZKSTARK_AMD_H
#define ZKSTARK_AMD_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>   /* ZK_STRUCT_INIT */

#ifdef __cplusplus
extern "C" {
#endif

#define ZK_FIELD_P 3221225473u

enum zk_status {
    ZK_OK = 0,
    ZK_ERR_INVALID = -1,  /* bad argument (size not a power of two, out of range, ...) */
    ZK_ERR_HIP = -2,      /* HIP runtime / kernel failure */
    ZK_ERR_NOMEM = -3,
    ZK_ERR_STATE = -4,    /* stage called out of order */
    ZK_ERR_BUFFER = -5,   /* caller buffer too small */
    ZK_ERR_VERIFY = -6,   /* proof rejected (reference: panic in Proof::verify) */
    ZK_ERR_CHECK = -7     /* prover self-check failed (reference: assert_eq! in prover.rs) */
};

typedef struct zk_ctx zk_ctx;
typedef struct zk_channel zk_channel;   /* Channel (channel.rs:6-37), see below */

/* Merkle hash.  SHA-256 is the reference's (merkle.rs:1-2) and the default everywhere.  The
 * field-native hash (a Poseidon2-style permutation over GF(P), csrc/fieldhash.hpp) is the build's
 * own definition for BASELINE.json configs[4]; it has no reference counterpart.  The transcript
 * (channel.rs) always uses SHA-256.  Functions with an _ex suffix take the selector.
 * ZK_HASH_BLAKE2S is unkeyed BLAKE2s-256 (RFC 7693; csrc/blake2s.hpp): a leaf is the hash of its slots, 4 bytes
 * big-endian each (the message the SHA-256 leaf hashes), a node the hash of left || right -- one compression either way, and the 32
 * bytes in roots, paths and proofs are hashlib.blake2s(msg).digest().  Proof layouts and lengths do not depend on the hash.  Accepted by
 * zk_ctx_set_hash (with every setting of queries, grinding, folding factor, coset leaves and early stop; hence by zk_prove,
 * zk_prove_resident, zk_prove_channel and zk_prove_many), the CPU verifiers zk_verify_ex, zk_verify_queries, zk_verify_grind,
 * zk_verify_coset and zk_verify_stop (the general one: every setting, fold_log 1 and stop_log 0 included), zk_compute_root_from_path_ex,
 * zk_compute_root_from_coset, zk_dev_merkle_build_ex, zk_merkle_build_host_ex and zk_probe_hash_chain.  Not built yet, refused with
 * ZK_ERR_INVALID: zk_verify_check and zk_verify_fold (they keep the two hashes they were defined with; use zk_verify_stop), zk_batch_set_hash, zk_verifier_set_hash, zk_shard_set_hash, zk_tail_run, zk_dev_merkle_build_interleaved,
 * zk_dev_merkle_commit*, zk_dev_merkle_build_chunk and zk_dev_merkle_finish.  Speed against SHA-256: not timed yet
 * (tools/hash_kinds_bench.py). */
enum zk_hash_kind { ZK_HASH_SHA256 = 0, ZK_HASH_FIELD = 1, ZK_HASH_BLAKE2S = 2 };

const char *zk_last_error(void);
const char *zk_version(void);

/* ---- ABI version and caller-allocated structs -------------------------------------------------------------------
 * The reference has no FFI, so the rules of this seam are the build's own:
 *   - ZK_ABI_VERSION changes whenever an exported signature or the layout of a struct below changes incompatibly; a caller
 *     compiled against this header checks zk_abi_version() == ZK_ABI_VERSION once at start-up (the C programs under examples/ and tests/ do);
 *   - every struct the CALLER allocates (zk_transcript_info, zk_kernel_stat, zk_shard_options, zk_shard_stats,
 *     zk_shard_plan_info, zk_chain_probe) starts with `uint32_t struct_size`, which the caller sets to sizeof(the struct) as
 *     its own compiler sees it (ZK_STRUCT_INIT zeroes the struct and sets it) BEFORE every call, for outputs as well as for
 *     inputs.  The library reads / writes at most struct_size bytes and refuses (ZK_ERR_INVALID, zk_last_error names the
 *     struct and both sizes) a size of 0 or one below the struct's size in ABI version 6 (the first with this rule): a
 *     caller compiled against an older, smaller layout gets an error instead of shifted fields or a stack overwrite; a size
 *     between a published layout and the next (zk_transcript_info: 1244 bytes in version 6, 1256 with the grinding fields)
 *     is refused too, as no header ever had it;
 *   - new fields are appended at the END only, so a caller compiled against a smaller (>= version 6) layout keeps working:
 *     input fields it does not know are taken as 0 (= default), output fields it does not know are not written. */
#define ZK_ABI_VERSION 6u
uint32_t zk_abi_version(void);
#define ZK_STRUCT_INIT(ptr) (memset((ptr), 0, sizeof *(ptr)), (ptr)->struct_size = (uint32_t)sizeof *(ptr))
/* Hash of the sources and headers the library was built from (zkstark_amd/build.py: source_hash()); loaders
 * compare it with the tree to refuse a stale binary. */
const char *zk_build_hash(void);
/* How the host thread of the one-call provers hashes its share of the Merkle trees (the top 8 levels of every SHA-256
 * tree and the FRI layers of <= 2^9 values, csrc/host_sha.cpp; merkle.rs:14-51 is the definition either way):
 * 0 = portable code (then the provers leave every level to the device), 1 = x86 SHA extensions, 2 = SHA extensions plus
 * levels of >= 16 nodes sixteen at a time on AVX-512 registers.  Decided once from the CPU. */
int zk_host_hash_mode(void);
/* Restricts the host's hashing to `mode` (0, 1 or 2 as above; never more than the CPU has): 0 makes later contexts
 * leave every tree level to the device, 1 keeps the SHA unit but not the AVX-512 path (A/B measurements, tests).
 * Process-wide; call it while no prover is running and before the contexts it should affect are created. */
int zk_host_set_hash_mode(int mode);

/* ---- scalar field helpers on the host: field.rs:8-211 ------------------- */
uint32_t zk_field_add(uint32_t a, uint32_t b);       /* field.rs:99-111 */
uint32_t zk_field_sub(uint32_t a, uint32_t b);       /* field.rs:113-132 */
uint32_t zk_field_mul(uint32_t a, uint32_t b);       /* field.rs:134-167 */
uint32_t zk_field_neg(uint32_t a);                   /* field.rs:198-203 */
uint32_t zk_field_inv(uint32_t a);                   /* field.rs:205-210 */
uint32_t zk_field_pow(uint32_t a, uint32_t e);       /* field.rs:26-38 */
uint32_t zk_field_from_u32(uint32_t v);              /* field.rs:20-24 */
uint32_t zk_field_from_i32(int32_t v);               /* field.rs:10-18: v < 0 is -(|v| mod P) */
/* field.rs:165-177: a * b^-1.  b = 0 (mod P): the reference panics; returns 0 and sets zk_last_error. */
uint32_t zk_field_div(uint32_t a, uint32_t b);
/* field.rs:89-94 Rem<u32>: (residue of a) % rhs as a field element.  rhs = 0: the reference panics; returns 0 and
 * sets zk_last_error. */
uint32_t zk_field_rem(uint32_t a, uint32_t rhs);
uint32_t zk_field_generator(void);                   /* field.rs:52-86: the same search (first call), -> 5 */
uint32_t zk_field_root_of_unity(uint32_t log_order); /* prover.rs:48-49 */
uint32_t zk_field_order(uint32_t a);                 /* field.rs:45-49 (via P-1 = 3*2^30, not brute force) */

/* ---- the quadratic extension E = F_P[u] / (u^2 - 5) on the host ------------
 * 5 = zk_field_generator() is a non-residue.  An element is a pair (c0, c1) = c0 + c1 u;
 * (a0 + a1 u)(b0 + b1 u) = (a0 b0 + 5 a1 b1) + (a0 b1 + a1 b0) u.  Inputs are any u32 (reduced mod P as zk_field_* reduce),
 * results canonical; out may alias an input.  ZK_OK or ZK_ERR_INVALID (null argument; the inverse of zero). */
int zk_ext_mul(const uint32_t a[2], const uint32_t b[2], uint32_t out[2]);
int zk_ext_inv(const uint32_t a[2], uint32_t out[2]);
int zk_ext_pow(const uint32_t a[2], uint64_t e, uint32_t out[2]);

/* ---- context ------------------------------------------------------------- */
/* Allocates HBM for a proof with trace group size n = 2^log_n and blow-up
 * B = 2^log_blowup (reference literals: 10 and 3, prover.rs:48-57), builds the
 * twiddle and denominator tables.  One-time cost; zk_ctx_setup_ms reports it. */
int zk_ctx_create(int device, uint32_t log_n, uint32_t log_blowup, zk_ctx **out);
int zk_ctx_destroy(zk_ctx *ctx);
double zk_ctx_setup_ms(const zk_ctx *ctx);
size_t zk_ctx_device_bytes(const zk_ctx *ctx);
int zk_ctx_sync(zk_ctx *ctx);
/* Number of decommitment queries of later zk_prove* calls (1..64; default 1 = the reference,
 * prover.rs:263).  With q > 1 the q raw indices are drawn in a row and each query's openings are
 * committed in turn; q = 1 is byte-identical to the reference format. */
int zk_ctx_set_queries(zk_ctx *ctx, uint32_t n_queries);
/* Proof-of-work grinding of later zk_prove* (zk_prove_resident, zk_prove_channel, zk_prove_many; DESIGN.md "Grinding"; the
 * reference has none).  grind_bits = g in 0..32, default 0.  g = 0: no nonce, every byte as without this call.  g > 0: after the
 * free term is committed (prover.rs:254) the prover finds the SMALLEST u64 w such that SHA-256(S || le64(w)) begins with g zero
 * bits (S = the channel state; bits read MSB-first from byte 0, as zk_channel_get_u32 reads the state), commits le64(w) (bincode
 * u64: 8 bytes between the free term and the first query raw) and draws the queries as before.  A cheating prover then redoes
 * 2^g hashes per query set it tries: conjectured security bits ~ n_queries * log_blowup + g.  Small g is searched on the
 * calling thread, larger g on the device (csrc/grind.hip); the nonce is the same either way.  The sharded prover (zk_shard_*)
 * does not grind. */
int zk_ctx_set_grinding(zk_ctx *ctx, uint32_t grind_bits);
/* Opt-in reference self-checks.  The reference asserts its way through generate_proof; with on != 0 the same
 * checkpoints run inside every later zk_prove* on the data as it sits in HBM: the interpolant passes through every
 * trace point (prover.rs:64-66), every constraint division is exact and deg cp = n - 1 (prover.rs:148-159, :169), every
 * FRI layer has its asserted degree (prover.rs:228-251).  The first checkpoint that fails is named in a ZK_ERR_CHECK
 * (zk_last_error).  Off (default): only the last-layer check of prover.rs:238 runs. */
int zk_ctx_set_checks(zk_ctx *ctx, int on);
/* Selects the Merkle hash of every later zk_merkle_commit / zk_prove* on this context. */
int zk_ctx_set_hash(zk_ctx *ctx, int hash_kind);
/* Division of the latency-bound end of zk_prove* between device and host.  A Merkle level is a chain of dependent
 * hashes (merkle.rs:40-46): ~4.6 us on a GPU wave (2 293 issue slots of 4 cycles at the ~2.1 GHz the chip holds), ~31 ns
 * per node on a CPU core with SHA extensions.  With top_log = H > 0 the device builds every SHA-256 tree with more than
 * 2^H leaves down to its 2^H nodes of depth H (a smaller tree: one level below its leaves) and the host hashes the nodes
 * above: the calling thread alone for H <= 8, a team of 2^(H-8) threads (one 256-digest sub-tree each, the workers spin
 * between the commitments of a proof) for H = 9, 10.  With tail_log = T > 0, FRI layers of <= 2^T values
 * (polynomial.rs:385 fold + merkle.rs:14 tree) are computed by the calling thread as well.  Everything the host built
 * is copied into the device arrays before the call returns, so zk_layer_read / zk_merkle_path see complete trees.
 * Default: (8, 9) when the CPU has SHA extensions, else (0, 0) = all on the device (H, T <= 10; T > 0 needs H > 0).
 * zk_merkle_commit hands over its tree top in the same way; the field hash always runs on the device.  Results are
 * identical for every setting. */
int zk_ctx_set_host_levels(zk_ctx *ctx, uint32_t top_log, uint32_t tail_log);
int zk_ctx_get_host_levels(const zk_ctx *ctx, uint32_t *top_log, uint32_t *tail_log);
/* Early launch (round 6).  A proof is a chain of commitments: digests to the host, root into the channel, challenge out, the next
 * layer's launches (prover.rs:198-225).  With on != 0, zk_prove* enqueues the fold + commit launches of the NEXT FRI round before it
 * waits for the current commitment, behind a command-processor wait on a host word (hipStreamWaitValue32), and releases them with
 * one store once the challenge is drawn: the launch call and ~2.5 us of dispatch latency per commitment leave the critical path.
 * Results are identical either way.  Off by default: measured inside one build at nothing outside the spread for a 2^24 proof,
 * -1.5 % for a 2^20 proof, -5 % at the reference's own size (profiles/r06_ab_early_launch.txt); worth switching on for small
 * domains proved one at a time.  Contexts that share a GPU (zk_prove_many) should leave it off: a stream that waits on its gate
 * holds the hardware queue another context's stream may be mapped to.  zk_ctx_get_early_launch: 1 when on AND supported. */
int zk_ctx_set_early_launch(zk_ctx *ctx, int on);
int zk_ctx_get_early_launch(const zk_ctx *ctx);
/* FRI folding factor 2^fold_log between commitments, fold_log in 1..3 (default 1 = the reference, which folds by two and commits
 * every layer: prover.rs:198-225; a proof made with the default is byte for byte what it was).  The log_n rounds are taken in groups
 * of fold_log (the last may be shorter): a group draws ONE challenge beta (prover.rs:200), its output is that many successive
 * folds (polynomial.rs:385 + prover.rs:204-211) with beta, beta^2, beta^4, computed in one pass, and only that output is committed
 * (prover.rs:214, :224), under the reference's layer id (1 + round).  Per query a group opens the 2^steps coset values of its input
 * layer and their paths -- the tuple of prover.rs:280-289 widened -- and the verifier (proof.rs:101-148 widened) folds them down
 * to the next group's value.  A query still tests one coset per committed layer, so the conjectured security per query is
 * unchanged; the price is proof size (leaves stay one value wide, so 2^steps paths per group): at domain 2^24 with one query
 * 23 280 / 23 560 / 31 008 bytes for fold_log 1 / 2 / 3, with 32 queries 719 044 / 739 164 / 981 964 (zk_proof_data_len_fold).
 * Trees per 2^24 proof: 23 / 13 / 9.  Honoured by zk_prove, zk_prove_resident, zk_prove_channel and zk_prove_many with every other
 * option.  With fold_log > 1: every FRI layer is folded on the device (the host FRI tail of zk_ctx_set_host_levels is left out;
 * the tree-top hand-over works as usual and results are identical for every setting); early launch is not used and
 * zk_ctx_get_early_launch answers 0; zk_last_transcript has beta_raw[r0] = the challenge of the group that starts at round r0 and
 * roots[id] for committed ids, the rest zero; zk_layer_read / zk_merkle_node(s) / zk_merkle_path of an id the proof did not
 * materialise return ZK_ERR_STATE.  Measured, K = 1, 2, 3 interleaved in one process (profiles/fold_arity_bench.txt): 5.69 / 4.41 /
 * 3.95 ms per proof at domain 2^24, 0.952 / 0.771 / 0.640 ms at 2^20.  NOT faster everywhere: at the reference's size (domain 2^13)
 * 0.274 / 0.296 / 0.264 ms -- fold_log 2 is 8 % SLOWER than the default there and fold_log 3 only 4 % faster, because the default
 * folds the small layers on the host thread and fuses every fold into its leaf hashing, while a folded proof pays one fold launch
 * and one tree launch per group (docs/LOG.md "Folding factor").
 * zk_verifier_* follows with zk_verifier_set_fold; zk_shard_* / zk_tail_* stay at factor 2. */
int zk_ctx_set_fold(zk_ctx *ctx, uint32_t fold_log);
uint32_t zk_ctx_get_fold(const zk_ctx *ctx);
/* Coset leaves: off by default (with it off every byte, launch and allocation is what it was); valid with every fold_log, hash,
 * query count, grinding and zk_prove_channel.  With it on, the tree over the input layer of group j (id 1 + r0, len = N >> r0 values,
 * s = 2^steps_j) has len / s leaves; leaf c holds the slots u = 0 .. s-1, slot u = layer[c + u len / s] -- the coset a query opens there --
 * so a group opens ONE leaf of s values and ONE path of L - r0 - steps digests instead of s values and s paths.  Leaf hash: SHA-256 over
 * the s slots, 4 bytes big-endian each (one block), BLAKE2s-256 over the same message, or the field hash's compression of
 * (slot_0 .. slot_{s-1}, 0, ..., 0, s); s = 1 is the
 * one-value leaf; inner nodes are unchanged.  Tree 0 (f) and the tree over the last layer (never opened) keep one-value leaves; the
 * layers stay in natural order.  Per query: the three f tuples as ever, NO separate cp(x) tuple (group 0's leaf contains it), then per
 * group the s slot values in slot order, a u64 count and the path for leaf x % (len / s).  Length: zk_proof_data_len_coset; verifier:
 * zk_verify_coset.  At domain 2^24 with one query 12 252 / 7 332 / 5 644 bytes for fold_log 1 / 2 / 3 (plain leaves 23 280 / 23 560 /
 * 31 008), with 32 queries 366 148 / 219 868 / 170 316.  A tree over len / s leaves costs 2 len / s hashes instead of 2 len (a leaf of up
 * to 8 words is still one compression), hashed by coset_leaf_hash_kernel and the inner build.  Every layer is a device layer, for
 * fold_log 1 too: the host FRI tail, the fold and the composition fused into leaf hashing and early launch apply only with coset
 * leaves off (zk_ctx_get_early_launch answers 0); the tree-top hand-over works as usual on the smaller trees (a tree of at most
 * 2^top_log LEAVES hands over one level below its leaves) and results are identical for every setting.  zk_merkle_node(s) /
 * zk_merkle_path address a coset tree by its own leaves: 2 len / s - 1 nodes, leaf index < len / s, L - r0 - steps digests.
 * Measured: see DESIGN.md 7d.
 * zk_verifier_* checks such proofs in batches with zk_verifier_set_coset_leaves; zk_batch_* makes them with
 * zk_batch_set_coset_leaves.
 * NOT covered: zk_shard_* / zk_tail_* keep one-value leaves. */
int zk_ctx_set_coset_leaves(zk_ctx *ctx, int on);
int zk_ctx_get_coset_leaves(const zk_ctx *ctx);
/* Early stop: stop_log = D, default 0 (with 0 every byte, launch and allocation is what it was; the reference folds down to a
 * constant, prover.rs:198-254); valid with every fold_log, leaf format, hash, query count, grinding, zk_prove_channel and zk_prove_many.
 * With D > 0 only the first R' = log_n - D rounds are folded, in the groups of R' (G' = ceil(R' / fold_log), the last possibly shorter).
 * The output of the last group, layer id 1 + R', holds M = 2^(D + log_blowup) evaluations of a polynomial p of degree < 2^D at
 * X_i = (w h^i)^(2^R'), natural order.  It is NOT committed as a tree: the prover sends the 2^D monomial coefficients of p in X.  Header, in
 * wire order: f_root, alpha0..2, root0, then beta_j, root_{j+1} for j = 0 .. G'-2, then beta_{G'-1}, then c_0 .. c_{2^D - 1} (canonical
 * residues, 4 bytes little-endian each, committed to the channel in ONE piece of 4 * 2^D bytes -- they take the place of the last root
 * and the free term), then the nonce (searched on the state after the coefficients) and the query raws.  Per query exactly the tuples of
 * the G' groups, plain or coset; with coset leaves the tree over the last group's input has that group's cosets as leaves, and no tree has
 * the stopped layer's values as leaves.  Length: zk_proof_data_len_stop; verifier: zk_verify_stop.
 * Limits: D <= 8, D <= log_n - 1 (at least one round is folded), D + log_blowup <= 12 (the stopped layer fits one workgroup's LDS);
 * anything else is ZK_ERR_INVALID and the setting is unchanged.
 * Soundness: a query still tests one coset per committed layer, and the degree bound of the final polynomial holds by construction --
 * 2^D coefficients are a polynomial of degree < 2^D, where the reference's constant is one of degree < 1.
 * The prover: fri_final_poly_kernel (one workgroup: inverse NTT of the M values in LDS, scaling by M^-1 s^-k, s = w^(2^R')) and one copy of
 * 2^D + 1 words replace the D last fold + tree launches and the free term.  If a coefficient of degree >= 2^D is non-zero the proof fails
 * with ZK_ERR_CHECK "final FRI layer has degree >= 2^D" (the analogue of the prover.rs:238 check).  With zk_ctx_set_checks the degree
 * checkpoints run for the layers that exist.  With D > 0 every layer is a device layer and every fold_log, 1 without coset leaves too,
 * takes the grouped round loop: the fold fused into leaf hashing, early launch and the host FRI tail do not apply
 * (zk_ctx_get_early_launch answers 0) -- that is the price at large domains for fold_log 1.  zk_last_transcript: free_term = c_0,
 * roots[1 + R'] and everything past it zero.  After a stopped proof zk_layer_read of an id beyond 1 + R', and zk_merkle_node(s) /
 * zk_merkle_path of a tree id >= 1 + R' (layer 1 + R' has no tree), return ZK_ERR_STATE; a later D = 0 proof materialises everything again.
 * Not run or timed on a GPU yet (tools/fri_stop_bench.py is the tool; DESIGN.md 7d "Early stop"): fold_log 1 without coset leaves may
 * well be slower with D > 0 at large domains.
 * zk_verifier_* checks such proofs in batches with zk_verifier_set_fri_stop; zk_batch_* makes them with zk_batch_set_fri_stop.
 * NOT covered: zk_shard_* and zk_tail_* keep folding down to a constant.
 * zk_ctx_get_fri_stop: the current D, 0 for a null context.  zk_ctx_final_poly: the coefficients of the last proof (count <- their
 * number; ZK_ERR_BUFFER if cap is smaller, ZK_ERR_STATE before the first proof); with D = 0 count is 1 and out[0] the free term. */
int zk_ctx_set_fri_stop(zk_ctx *ctx, uint32_t stop_log);
uint32_t zk_ctx_get_fri_stop(const zk_ctx *ctx);
int zk_ctx_final_poly(const zk_ctx *ctx, uint32_t *out, size_t cap, size_t *count);
/* Merkle caps: cap_log = c, default 0 (with 0 every byte, launch and allocation is what it was); 0 <= c <= 8, anything else is
 * ZK_ERR_INVALID and the setting is unchanged; a zk_tail_create context answers ZK_ERR_STATE.  Valid with every hash, fold_log, leaf
 * format, stop_log, query count, grinding, host-levels setting and early launch, in zk_prove, zk_prove_resident, zk_prove_channel and
 * zk_prove_many.  A tree over 2^lg leaves (a coset leaf counts once) is committed by the 2^ce digests of depth ce = min(c, lg - 1) --
 * heap nodes 2^ce - 1 .. 2^(ce+1) - 2, left to right, 32 bytes each in the byte form of a root, ONE channel commit -- in place of its root:
 * f, cp (or group 0's input tree), every group output that gets a tree, and the never-opened last tree when stop_log = 0.  A path into the
 * tree carries the lg - ce siblings from the leaf up to depth ce + 1, behind a u64 count of lg - ce; the verifier hashes upward lg - ce times
 * and compares with cap entry leaf >> (lg - ce).  Nothing above depth ce is hashed by the device, the host thread or the verifier: the
 * build is handed over at depth max(ce, the host's share) and the host reduces from there down to ce only.  Length:
 * zk_proof_data_len_cap; verifier: zk_verify_cap.  The cap pays with several queries only: the head grows by 32 (2^ce - 1) bytes per
 * tree, each path shrinks by 32 ce.
 * After a proof with c > 0: zk_last_transcript's roots[id] is all zero for a tree with ce > 0 and zk_ctx_merkle_cap has its digests; the
 * heap of such a tree above depth ce is not defined (it may hold an earlier proof's nodes), so zk_merkle_node / zk_merkle_nodes of an
 * index above the cap and zk_merkle_path of that tree return ZK_ERR_STATE.  The stage-by-stage API (zk_merkle_commit*, zk_dev_*)
 * ignores the setting and builds whole trees.
 * zk_verifier_* checks such proofs in batches with zk_verifier_set_merkle_cap.
 * zk_batch_* makes the same proofs in batches with zk_batch_set_merkle_cap.
 * NOT covered: zk_shard_* and zk_tail_* have no cap setting yet.
 * zk_ctx_get_merkle_cap: the current c, 0 for a null context.  zk_ctx_merkle_cap_log: the ce tree `tree` was last built down to.
 * zk_ctx_merkle_cap: what the last one-call proof committed for `tree`, 32 * 2^ce bytes (ce = 0: the root); ZK_ERR_BUFFER if out_len is
 * smaller, ZK_ERR_STATE before the first proof or for a tree the proof did not build. */
int zk_ctx_set_merkle_cap(zk_ctx *ctx, uint32_t cap_log);
/* Challenges in the quadratic extension E = F_P[u] / (u^2 - 5) (zk_ext_*; DESIGN.md 7j fixes the format): ext_log = 1, default 0, from the
 * next one-call proof on (zk_prove, zk_prove_resident, zk_prove_channel, zk_prove_many), with every fold_log, leaf format, fri_stop,
 * merkle_cap, query count, grinding, hashes 0 and 1 and host levels.  The trace and f stay in the base field; the alphas, cp, every beta
 * and every FRI layer are in E.  With ext on every folding factor and leaf format takes the grouped round loop (no fused leaf launches,
 * early launch or host FRI tail: zk_ctx_get_early_launch answers 0), the trees over cp and the FRI layers are row trees over the layer's two planes, and the reference
 * self-checks (zk_ctx_set_checks) hold both planes to the degree bound.  The setter sizes the second planes and the decommitment buffers
 * when called, both ways: with ext_log = 0 zk_ctx_device_bytes, every launch and every byte are what they were.  It drops the layers of
 * the last proof.  ZK_ERR_INVALID for ext_log > 1 (2, the quartic extension, is reserved) and for ext_log = 1 with BLAKE2s, which has no
 * row leaf (zk_ctx_set_hash(2) with ext on is refused the same way); ZK_ERR_STATE while a proof runs on the context (a proof started
 * while the setter runs gets ZK_ERR_STATE instead).  After an ext proof zk_last_transcript holds component 0 of every challenge in the
 * fields it has, zk_ctx_ext_challenges the component-1 raws (alpha0.c1, alpha1.c1, alpha2.c1, then one per group; *count = 0 after a
 * base-field proof), zk_ctx_final_poly the words of the free term or the coefficients in wire order, and layers with id >= 1 are not
 * materialised for zk_layer_read (ZK_ERR_STATE).  Proofs: zk_proof_data_len_ext bytes, checked by zk_verify_ext.
 * The stage-by-stage context API (zk_compose, zk_fri_fold, zk_merkle_commit, ...) stays base-field. */
int zk_ctx_set_ext(zk_ctx *ctx, uint32_t ext_log);
uint32_t zk_ctx_get_ext(const zk_ctx *ctx);
int zk_ctx_ext_challenges(const zk_ctx *ctx, uint32_t *out, size_t cap, size_t *count);
uint32_t zk_ctx_get_merkle_cap(const zk_ctx *ctx);
uint32_t zk_ctx_merkle_cap_log(const zk_ctx *ctx, uint32_t tree);
int zk_ctx_merkle_cap(const zk_ctx *ctx, uint32_t tree, uint8_t *out, size_t out_len);
/* The HIP stream every stage is enqueued on (hipStream_t). */
void *zk_ctx_stream(zk_ctx *ctx);

/* ---- trace: prover.rs:32-42 ---------------------------------------------- */
/* a0, a1, a[i] = a[i-2]^2 + a[i-1]^2 on the host (serial recurrence). */
int zk_trace_fibsq(uint32_t a0, uint32_t a1, size_t count, uint32_t *out);
/* Uploads the n-1 trace values (prover.rs:60 interpolates exactly n-1 points). */
int zk_trace_upload(zk_ctx *ctx, const uint32_t *trace, size_t count);

/* ---- stages on context-resident data --------------------------------------- */
/* lagrange (polynomial.rs:337) + solve over w*h^i (polynomial.rs:49, prover.rs:60-70):
 * layer 0 <- f(w h^i), i < N, natural order. */
int zk_lde(zk_ctx *ctx);
/* Merkle::new over a layer (merkle.rs:14-51; prover.rs:81, :176, :214); root = node 0.  Returns once the root is known.  With
 * a host hand-over (zk_ctx_set_host_levels) the device copy of the nodes this thread hashed (the top 8 levels) is ordered on
 * the stream by the next call that reads trees or layers from the device (zk_merkle_node, zk_merkle_path, zk_layer_read,
 * zk_ctx_sync, zk_ctx_stream), not by this one: a loop of commitments does not pay a copy launch per iteration. */
int zk_merkle_commit(zk_ctx *ctx, uint32_t layer, uint8_t root_out[32]);
/* The tree over a layer of len values with 2^steps-wide coset leaves (zk_ctx_set_coset_leaves): leaf c < len / 2^steps holds
 * layer[c + u len / 2^steps], u < 2^steps.  steps 0..3 with at least two leaves; steps = 0 is zk_merkle_commit. */
int zk_merkle_commit_coset(zk_ctx *ctx, uint32_t layer, uint32_t steps, uint8_t root_out[32]);
/* Constraint quotients and their random combination (prover.rs:101-173):
 * layer 1 <- cp(w h^i).  alpha_raw are the raw u32 challenges (prover.rs:163-165). */
int zk_compose(zk_ctx *ctx, const uint32_t alpha_raw[3]);
/* fri() + squared half domain + re-evaluation (polynomial.rs:385, prover.rs:198-211):
 * layer 2+round <- fold(layer 1+round, beta). */
int zk_fri_fold(zk_ctx *ctx, uint32_t round, uint32_t beta_raw);
/* `steps` (1..3) successive folds with the challenges beta, beta^2, beta^4 in one pass (zk_ctx_set_fold):
 * layer 1+round+steps <- fold^steps(layer 1+round); round + steps <= log_n.  steps = 1 gives what zk_fri_fold gives. */
int zk_fri_fold_multi(zk_ctx *ctx, uint32_t round, uint32_t steps, uint32_t beta_raw);
/* The stage behind zk_ctx_set_fri_stop (fri_final_poly_kernel): FRI layer id `layer` >= 1, M = layer size <= 4096 values at
 * X_i = (w h^i)^(2^(layer-1)).  coef_out[k], k < M <- the monomial coefficients in X of the polynomial of degree < M through them
 * (canonical residues); *high_nonzero <- how many coefficients with k >= bound are non-zero (bound >= M: 0).  A larger layer or
 * layer 0: ZK_ERR_INVALID; a layer the last proof did not materialise: ZK_ERR_STATE. */
int zk_fri_final_poly(zk_ctx *ctx, uint32_t layer, uint32_t bound, uint32_t *coef_out, uint32_t *high_nonzero);
/* Small device->host reads (decommit, tests). */
int zk_layer_read(zk_ctx *ctx, uint32_t layer, size_t offset, size_t count, uint32_t *out);
int zk_layer_write(zk_ctx *ctx, uint32_t layer, size_t offset, size_t count, const uint32_t *in);
/* Index<usize> for Merkle (merkle.rs:74-79). */
int zk_merkle_node(zk_ctx *ctx, uint32_t tree, size_t index, uint8_t out[32]);
/* Nodes [first, first + count) of a tree in one copy, 32 bytes each as zk_merkle_node (out: 32 * count bytes). */
int zk_merkle_nodes(zk_ctx *ctx, uint32_t tree, size_t first, size_t count, uint8_t *out);
/* Merkle::trace (merkle.rs:54-71): sibling of the leaf first, child of the root last.
 * out holds 32 * log2(m) bytes; *path_len receives log2(m). */
int zk_merkle_path(zk_ctx *ctx, uint32_t tree, size_t leaf, uint8_t *out, size_t *path_len);

/* ---- whole prover: generate_proof (prover.rs:9-293) ------------------------- */
/* Runs from "trace resident on device" (zk_trace_upload) to "proof bytes on host".
 * proof_out receives Channel.data (channel.rs:8), state_out Channel.state
 * (channel.rs:34-36), i.e. the two fields of Proof (proof.rs:5-8). */
int zk_prove_resident(zk_ctx *ctx, uint8_t *proof_out, size_t cap, size_t *proof_len,
                      uint8_t state_out[32]);
/* generate_proof(channel: Channel) -> Proof (prover.rs:9) literally: proves the resident trace on the CALLER'S
 * channel (channel.rs:6-37).  Every commitment is appended to `ch` and every challenge is drawn from it, so a
 * channel that already holds a transcript prefix yields the proof bound to that prefix; Proof{state, data}
 * (proof.rs:5-8, channel.rs:34-36) is then zk_channel_state / zk_channel_data.  With a fresh channel
 * (main.rs:19) the bytes equal zk_prove_resident's. */
int zk_prove_channel(zk_ctx *ctx, zk_channel *ch);
/* zk_prove_resident on `count` (1..16) distinct contexts at once, one host thread each: the latency-bound
 * phases of one proof overlap the hashing of the others on the same GPU.  Proof i goes to
 * proofs_out + i*stride (stride >= the proof length), its length to lens_out[i], its state to
 * states_out + 32*i. */
int zk_prove_many(zk_ctx *const *ctxs, size_t count, uint8_t *proofs_out, size_t stride, size_t *lens_out,
                  uint8_t *states_out);
/* zk_trace_upload + zk_prove_resident. */
int zk_prove(zk_ctx *ctx, const uint32_t *trace, size_t count, uint8_t *proof_out, size_t cap,
             size_t *proof_len, uint8_t state_out[32]);
/* Challenges and checkpoints of the last zk_prove* on this context (tests/diagnostics). */
typedef struct zk_transcript_info {
    uint32_t struct_size;   /* sizeof(zk_transcript_info), set by the caller (see "ABI version" above) */
    uint32_t alpha_raw[3];
    uint32_t beta_raw[32];
    uint32_t free_term;
    uint32_t query_raw;
    uint32_t public_last; /* a[n-2] */
    uint8_t roots[34][32]; /* trees 0 .. log_n + 1 */
    uint32_t grind_bits;   /* zk_ctx_set_grinding of that proof (0: no nonce) */
    uint64_t grind_nonce;  /* the nonce committed after the free term (grind_bits > 0) */
} zk_transcript_info;
int zk_last_transcript(const zk_ctx *ctx, zk_transcript_info *out);
/* Optional per-kernel timing with HIP events on the context stream.  class_mask selects
 * the kernel classes to bracket (bit i = class i below; 0 = off, the default), so a
 * benchmark can time only the dominant kernel inside its timed region. */
enum zk_kernel_class {
    ZK_K_NTT = 0,           /* ntt_pass_kernel (iNTT / LDE passes) */
    ZK_K_MERKLE_LEAF = 1,   /* merkle_subtree_kernel<leaf>: leaf hashes + k inner levels */
    ZK_K_MERKLE_INNER = 2,  /* merkle_subtree_kernel<inner> */
    ZK_K_MERKLE_TOP = 3,    /* merkle_wg_kernel: the latency-bound levels, workgroup-local */
    ZK_K_COMPOSE = 4,
    ZK_K_FOLD = 5,
    ZK_K_GATHER = 6,
    ZK_K_COUNT = 7
};
typedef struct zk_kernel_stat {
    uint32_t struct_size;   /* sizeof(zk_kernel_stat), set by the caller in out[0]: the stride of the array */
    uint32_t reserved;
    uint64_t launches;
    double ms;     /* summed launch durations */
    double bytes;  /* summed ALGORITHMIC bytes of those launches */
    double ops;    /* summed compulsory 32-bit VALU lane-ops (SHA-256 kernels; 0 elsewhere) */
} zk_kernel_stat;
int zk_ctx_set_profiling(zk_ctx *ctx, uint32_t class_mask);
/* Copies the accumulated statistics (count <= ZK_K_COUNT entries); reset != 0 clears them. */
int zk_kernel_stats(zk_ctx *ctx, zk_kernel_stat *out, size_t count, int reset);

/* ---- batched proving ---------------------------------
 * 2^log_batch independent proofs of one size (prover.rs:9-293 each, its own Channel each) computed in
 * lockstep: the layers of the batch are stored proof-major, so every stage is ONE launch of the kernels
 * a single proof uses on a domain batch times larger, and the trees of the batch are the bottom of one
 * heap whose nodes of depth log_batch are the per-proof roots.  Every proof is byte-identical to what
 * zk_prove returns for the same trace from a context with the batch's settings: hash, queries, grinding, folding factor
 * (zk_batch_set_fold), leaf format (zk_batch_set_coset_leaves; off by default) and early stop (zk_batch_set_fri_stop; 0 by default).  With coset leaves a tree over len values per
 * proof has len / s leaves per proof and the batch heap batch * len / s.  log_batch <= 10; (log_n, log_blowup) as for
 * zk_ctx_create (log_n >= 2, != 3), so every proof a batch produces can be checked by zk_verify*.  A batch of one (log_batch 0)
 * is a zk_ctx: every setter forwards to it. */
typedef struct zk_batch zk_batch;
int zk_batch_create(int device, uint32_t log_n, uint32_t log_blowup, uint32_t log_batch, zk_batch **out);
int zk_batch_destroy(zk_batch *b);
size_t zk_batch_size(const zk_batch *b);                    /* 2^log_batch */
/* As zk_ctx_set_queries (1..16 here) and zk_ctx_set_hash, for every proof of the batch. */
int zk_batch_set_queries(zk_batch *b, uint32_t n_queries);
int zk_batch_set_hash(zk_batch *b, int hash_kind);
/* As zk_ctx_set_grinding, for every proof of the batch: one launch searches the nonces of all proofs of the batch at once. */
int zk_batch_set_grinding(zk_batch *b, uint32_t grind_bits);
/* As zk_ctx_set_fold, for every proof of the batch: fold_log 1..3, default 1 (with it every byte, launch and allocation of
 * zk_batch_prove is what it was without this call).  With fold_log = K > 1 the rounds are taken in groups of K (the last may be
 * shorter); per group every proof draws ONE challenge from its own channel, one batched multi-fold launch produces layer
 * 1 + r0 + steps of the whole batch, one tree is built over it and the per-proof roots are committed under that id; the ids in
 * between are neither computed nor committed.  Every proof is byte for byte what zk_prove returns from a context with the same
 * (log_n, log_blowup, hash, n_queries, grind_bits, fold_log) and trace, its state too; its length is zk_proof_data_len_fold and it is
 * checked with zk_verify_fold, or in batches with zk_verifier_set_fold + zk_verifier_run.  After a folded zk_batch_prove, zk_batch_merkle_nodes of a tree id
 * the proof did not build returns ZK_ERR_STATE; a later proof with fold_log 1 materialises every id again.  The decommitment buffers
 * are re-sized here (a folded proof opens up to 8 values per group).  Device memory: the layers and trees of the skipped ids stay
 * allocated (the batch can go back to fold_log 1 at any time); fold_log > 1 adds 32 bytes per proof.
 * zk_batch_get_fold: the current fold_log, 0 for a null batch. */
int zk_batch_set_fold(zk_batch *b, uint32_t fold_log);
uint32_t zk_batch_get_fold(const zk_batch *b);
/* As zk_ctx_set_coset_leaves, for every proof of the batch: off by default (with it off every byte, launch and allocation of
 * zk_batch_prove is what it was without this call); any non-zero `on` means on, from the next zk_batch_prove on.  It combines with every
 * fold_log 1..3, hash, query count 1..16 and grinding.  With it on, proof p is byte for byte what zk_prove returns from a context with the
 * same (log_n, log_blowup, hash, n_queries, grind_bits, fold_log), zk_ctx_set_coset_leaves(ctx, 1) and the same trace, its state too; its
 * length is zk_proof_data_len_coset and it is checked with zk_verify_coset, or in batches with zk_verifier_set_coset_leaves.  The flow
 * is the one-call prover's: trees 0 (f) and 1 + log_n (last layer) keep one-value leaves; cp is composed by a launch of its own and
 * its tree has group 0's cosets as leaves; every group, for fold_log 1 too, is one batched multi-fold launch, and the tree over its
 * output has the next group's cosets as leaves (coset_leaf_hash_batch_kernel, then the inner build).  The tree-top hand-over to the
 * host threads goes by the per-proof leaf count; results are identical with zk_batch_set_host_levels 0 and 1.  The decommitment
 * buffers are re-sized here, and the 32 bytes per proof of the multi-fold are allocated if they are not there yet; if an
 * allocation fails the call fails as zk_batch_set_fold does and the batch keeps its format.  Refused with ZK_ERR_STATE while a
 * zk_batch_prove runs.  A null batch: ZK_ERR_INVALID.  Measured: see DESIGN.md 7d.
 * zk_batch_get_coset_leaves: 1 or 0, 0 for a null batch. */
int zk_batch_set_coset_leaves(zk_batch *b, int on);
int zk_batch_get_coset_leaves(const zk_batch *b);
/* As zk_ctx_set_fri_stop, for every proof of the batch: stop_log = D, default 0 (with 0 every byte, launch and allocation of
 * zk_batch_prove is what it was without this call), from the next zk_batch_prove on.  It combines with every fold_log 1..3, leaf format,
 * hash, query count 1..16 and grinding; the limits are zk_ctx_set_fri_stop's (D <= 8, D <= log_n - 1, D + log_blowup <= 12; anything else
 * is ZK_ERR_INVALID and the setting is unchanged).  With D > 0, proof p is byte for byte what zk_prove returns from a context with the same
 * (log_n, log_blowup, hash, n_queries, grind_bits, fold_log, coset leaves), zk_ctx_set_fri_stop(ctx, D) and the same trace, its state too;
 * its length is zk_proof_data_len_stop and it is checked with zk_verify_stop, or in batches with zk_verifier_set_fri_stop.  The flow is
 * the one-call prover's: only the first R' = log_n - D rounds are folded, in the groups of R'; every group, for fold_log 1 without coset
 * leaves too, is one batched multi-fold launch (the fold fused into leaf hashing does not apply); the last group's output, layer
 * 1 + R' of the batch, gets no tree, no hand-over and no root.  One launch of fri_final_poly_batch_kernel (4096 / M layers of
 * M = 2^(D + log_blowup) values per workgroup, one shared twiddle table) writes a compact [batch][1 + 2^D] table -- per proof its own
 * count of non-zero coefficients of degree >= 2^D, then c_0 .. c_(2^D - 1) -- and one copy brings it to the host; each proof's channel
 * commits its 4 * 2^D coefficient bytes in one piece.  A non-zero count fails the call with ZK_ERR_CHECK "proof p of the batch: final FRI
 * layer has degree >= 2^D" for the lowest such p.  After a stopped zk_batch_prove, zk_batch_merkle_nodes of a tree id >= 1 + R' returns
 * ZK_ERR_STATE; a later D = 0 proof materialises every id again.  The decommitment buffers are re-sized here, the 32 bytes per proof of
 * the multi-fold are allocated if they are not there yet, and (1 + 2^D) words per proof are allocated on the device and in pinned host
 * memory; if an allocation fails the call fails as zk_batch_set_fold does and the batch keeps its format and buffers.  Setting the D the
 * batch already has changes nothing.  Refused with ZK_ERR_STATE while a zk_batch_prove runs.  A null batch: ZK_ERR_INVALID.
 * What has been run and timed on a GPU is recorded in DESIGN.md 7d "Early stop in the batched prover" (tools/batch_stop_bench.py is the tool): fold_log 1
 * without coset leaves gives up the fused fold + leaf-hash launch with D > 0 and may well be slower than D = 0 at large domains.
 * zk_batch_get_fri_stop: the current D, 0 for a null batch. */
int zk_batch_set_fri_stop(zk_batch *b, uint32_t stop_log);
uint32_t zk_batch_get_fri_stop(const zk_batch *b);
/* Merkle caps in the batched prover (zk_ctx_set_merkle_cap has the format): cap_log = c, default 0, 0 <= c <= 8 (anything else:
 * ZK_ERR_INVALID, the setting unchanged), from the next zk_batch_prove on; refused with ZK_ERR_STATE while a zk_batch_prove or another
 * setter runs.  It combines with every fold_log, leaf format, stop_log, query count, grinding, host-levels setting and both hashes of
 * this class, and every proof of the batch is byte for byte the one zk_ctx_set_merkle_cap(c) + zk_prove makes of the same trace:
 * zk_proof_data_len_cap bytes (the stride of zk_batch_prove), checked with zk_verify_cap or zk_verifier_set_merkle_cap.  With c = 0
 * every byte, launch and allocation is what it was.  log_batch = 0 forwards to zk_ctx_set_merkle_cap.
 * In the batch heap of a tree (zk_batch_merkle_nodes) the cap of proof p is the 2^ce nodes from 2^(log_batch + ce) - 1 + p 2^ce on,
 * ce = min(c, lg - 1) for 2^lg leaves per proof.  Nothing above depth log_batch + ce is built by the device or the host: after a
 * zk_batch_prove with ce > 0 for a tree, zk_batch_merkle_nodes of an index below 2^(log_batch + ce) - 1 returns ZK_ERR_STATE.  A cap of
 * more than 2^10 digests per batch is posted to a pinned buffer of 64 + 32 * 2^(log_batch + ce of the f tree) bytes which the setter
 * allocates (counted in zk_batch_device_bytes) and c = 0 or zk_batch_destroy frees; on ZK_ERR_NOMEM the batch keeps its setting.
 * zk_batch_get_merkle_cap: the current c, 0 for a null batch.  zk_batch_merkle_cap_log: the ce of tree `tree` in the last zk_batch_prove.
 * zk_batch_merkle_cap: what proof `proof` of the last zk_batch_prove committed for `tree`, 32 * 2^ce bytes (an uncapped tree: its root);
 * ZK_ERR_INVALID for a tree or proof out of range, ZK_ERR_BUFFER if out_len is smaller, ZK_ERR_STATE before the first proof or for a
 * tree the proof did not build. */
int zk_batch_set_merkle_cap(zk_batch *b, uint32_t cap_log);
uint32_t zk_batch_get_merkle_cap(const zk_batch *b);
uint32_t zk_batch_merkle_cap_log(const zk_batch *b, uint32_t tree);
int zk_batch_merkle_cap(zk_batch *b, uint32_t tree, size_t proof, uint8_t *out, size_t out_len);
/* Challenges in E = F_P[u] / (u^2 - 5) in the batched prover (zk_ctx_set_ext has the format): ext_log = 1, default 0, from
 * the next zk_batch_prove on.  It combines with every fold_log, leaf format, stop_log, cap_log, query count, grinding, host-levels setting
 * and both hashes of this class, and every proof of the batch is byte for byte the one zk_ctx_set_ext(1) + zk_prove makes of the same
 * trace: zk_proof_data_len_ext bytes (the stride of zk_batch_prove), checked with zk_verify_ext or zk_verifier_set_ext.  With ext on
 * the layers with id >= 1 are two planes each (component 0 first, each plane the proof-major layer of the base batch), every fold_log
 * and leaf format takes the grouped round loop (no fused leaf launches), and a tree has as many leaves and nodes as without: the leaf
 * of a value of E hashes its two words.  The setter sizes the planes, the gather buffers, the per-proof constants of E and the tables of
 * the final polynomials when called, both ways (counted in zk_batch_device_bytes): with ext_log = 0, also after it was 1, every byte,
 * launch and allocation is what it was.  ZK_ERR_INVALID for ext_log > 1 (2, the quartic extension, is reserved) or a null batch;
 * ZK_ERR_STATE while a zk_batch_prove or another setter runs; the value it already has: ZK_OK, nothing reallocated; on ZK_ERR_NOMEM the
 * batch keeps its setting and buffers.  log_batch = 0 forwards to zk_ctx_set_ext.  Ext and shared proofs stay apart:
 * zk_batch_prove_shared on a batch with ext on answers ZK_ERR_STATE before any launch and leaves the batch usable.
 * zk_batch_get_ext: the current ext_log, 0 for a null batch. */
int zk_batch_set_ext(zk_batch *b, uint32_t ext_log);
uint32_t zk_batch_get_ext(const zk_batch *b);
/* on = 0: every tree level of the batch on the device (default: the host threads hash the top levels of each proof's
 * trees when the CPU has SHA extensions, as zk_ctx_set_host_levels).  Results are identical. */
int zk_batch_set_host_levels(zk_batch *b, int on);
/* Host threads that run the per-proof transcript steps and decommit hashing (default: hardware threads, at most 16).
 * Like every zk_batch_set_* / trace call it is refused with ZK_ERR_STATE while a zk_batch_prove runs on the batch (one batch is
 * used from one host thread at a time; the guard turns a misuse into an error instead of a freed pool under a running proof). */
int zk_batch_set_threads(zk_batch *b, uint32_t threads);
size_t zk_batch_device_bytes(const zk_batch *b);
/* traces: [batch][n-1] canonical residues (prover.rs:32-39 per proof), uploaded and kept resident. */
int zk_batch_set_traces(zk_batch *b, const uint32_t *traces);
/* The same traces generated on the device from seeds a0[p], a1[p] (one lane per trace). */
int zk_batch_gen_fibsq(zk_batch *b, const uint32_t *a0, const uint32_t *a1);
/* out[p] = a[n-2] of proof p: the public input its verifier needs (prover.rs:42, proof.rs:68). */
int zk_batch_public_last(const zk_batch *b, uint32_t *out);
/* proofs_out: [batch][stride] bytes, stride >= zk_proof_data_len(log_n, log_blowup); states_out:
 * [batch][32] (with q queries: zk_proof_data_len_queries; in general zk_proof_data_len_fold(log_n, log_blowup, n_queries, grind_bits,
 * fold_log); with coset leaves zk_proof_data_len_coset of the same arguments; with an early stop zk_proof_data_len_stop).  Fails with ZK_ERR_CHECK, naming the proof, if a trace
 * breaks the constraints. */
int zk_batch_prove(zk_batch *b, uint8_t *proofs_out, size_t stride, uint8_t *states_out);
/* ONE proof of the M = 2^log_batch resident traces (a "shared proof"), with the batch's current settings: the f trees of
 * zk_batch_prove, committed together, then a single FRI over the sum of the M composition polynomials, each taken with its own three
 * alphas and its own public_last.  Wire format: the 2^(log_batch + ce_f) digests of the f heap (statement p's cap: entries p 2^ce_f
 * onwards) in one commit, 3M alphas statement-major, then the header of a single proof from cp on; per query the three f tuples of every
 * statement in turn, then the cp tuple and the group tuples of a single proof.  *proof_len = zk_proof_data_len_shared of the settings
 * (also when the buffer is too small: ZK_ERR_BUFFER); state_out: the Channel.state.  Checked with zk_verify_shared and the
 * zk_batch_public_last values.  ZK_ERR_INVALID for log_batch = 0 (a batch of one makes a plain proof) or > 8, ZK_ERR_STATE while another
 * call runs on the batch, ZK_ERR_CHECK if some trace of the batch breaks the constraints (the sum does not tell which).  Afterwards
 * tree 0 answers zk_batch_merkle_nodes / zk_batch_merkle_cap as after zk_batch_prove; the ids >= 1 answer ZK_ERR_STATE until the next
 * zk_batch_prove. */
int zk_batch_prove_shared(zk_batch *b, uint8_t *proof_out, size_t cap, size_t *proof_len, uint8_t state_out[32]);
/* Nodes [first, first + count) of batch tree `tree` (a heap over batch * m_l leaves; proof p's tree is the subtree under node
 * 2^log_batch - 1 + p), 32 bytes each as zk_merkle_node.  Complete after zk_batch_prove that succeeded (after one that failed with
 * ZK_ERR_CHECK the tree levels built on the host threads were never copied to the device: the nodes read then are not that run's).  The
 * nodes 0 .. 2^log_batch - 2 above the per-proof roots belong to no proof; the prover never builds them, this call hashes them on the
 * host from the per-proof roots, with the Merkle hash of the last zk_batch_prove.  ZK_ERR_STATE for a tree id that the last
 * proof, folded by zk_batch_set_fold, did not build.  A tree the last proof built with coset leaves of 2^steps values is addressed by
 * its own heap: 2 * batch * (len >> steps) - 1 nodes, anything beyond is ZK_ERR_INVALID; the batch remembers the steps of each tree per
 * proof, so a later plain proof has full-size heaps again. */
int zk_batch_merkle_nodes(zk_batch *b, uint32_t tree, size_t first, size_t count, uint8_t *out);

/* ---- proof: proof.rs ------------------------------------------------------- */
/* Proof::verify (proof.rs:15-149) on the CPU (many proofs at once on the GPU: zk_verifier_run below), generalised from the literals
 * (1024, 8192, 10, 2338775057) to (log_n, log_blowup, public_last). */
int zk_verify(const uint8_t *proof, size_t len, uint32_t log_n, uint32_t log_blowup,
              uint32_t public_last);
int zk_verify_ex(const uint8_t *proof, size_t len, uint32_t log_n, uint32_t log_blowup,
                 uint32_t public_last, int hash_kind);
/* General form: hash selector, q queries, and (state != NULL) the transcript replay of zk_verify_strict. */
int zk_verify_queries(const uint8_t *proof, size_t len, const uint8_t *state, uint32_t log_n, uint32_t log_blowup,
                      uint32_t public_last, int hash_kind, uint32_t n_queries);
/* zk_verify plus a replay of the Fiat-Shamir channel over the proof bytes: every challenge must be
 * the one the transcript yields at that point and `state` (Proof.state, proof.rs:6, which the
 * reference stores but never checks) must be the final channel state.  SURVEY.md section 8f item 1. */
int zk_verify_strict(const uint8_t *proof, size_t len, const uint8_t state[32], uint32_t log_n,
                     uint32_t log_blowup, uint32_t public_last);
/* Proof::size (proof.rs:151-154). */
size_t zk_proof_size(size_t data_len);
size_t zk_proof_data_len(uint32_t log_n, uint32_t log_blowup);
size_t zk_proof_data_len_queries(uint32_t log_n, uint32_t log_blowup, uint32_t n_queries);
/* With grind_bits > 0: 8 bytes more (the nonce). */
size_t zk_proof_data_len_grind(uint32_t log_n, uint32_t log_blowup, uint32_t n_queries, uint32_t grind_bits);
/* Proofs made with zk_ctx_set_fold(fold_log): 32 + 12 + 32 + 36 G + 4 + (grind ? 8 : 0) + q (4 + 4 (12 + 32 L) + sum over the
 * G = ceil(log_n / fold_log) groups of 2^steps (12 + 32 (L - r0))).  fold_log = 1: zk_proof_data_len_grind.  0 for a fold_log outside 1..3. */
size_t zk_proof_data_len_fold(uint32_t log_n, uint32_t log_blowup, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log);
/* Proofs made with zk_ctx_set_coset_leaves: 32 + 12 + 32 + 36 G + 4 + (grind ? 8 : 0) + q (4 + 3 (12 + 32 L) + sum over the groups of
 * 4 s + 8 + 32 (L - r0 - steps)), s = 2^steps.  0 for a fold_log outside 1..3. */
size_t zk_proof_data_len_coset(uint32_t log_n, uint32_t log_blowup, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log);
/* Proofs made with zk_ctx_set_fri_stop(stop_log = D): 32 + 12 + 32 + 36 (G' - 1) + 4 + 4 * 2^D + (grind ? 8 : 0) + q (per-query bytes of
 * zk_proof_data_len_fold, or _coset when coset_leaves != 0, summed over the G' groups of log_n - D rounds only).  stop_log = 0: what
 * zk_proof_data_len_fold / _coset return.  0 for a fold_log outside 1..3 or a stop_log outside the limits of zk_ctx_set_fri_stop. */
size_t zk_proof_data_len_stop(uint32_t log_n, uint32_t log_blowup, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log,
                              int coset_leaves, uint32_t stop_log);
/* Proofs made with zk_ctx_set_merkle_cap(cap_log = c): zk_proof_data_len_stop of the other arguments, plus 32 (2^ce - 1) per committed
 * tree, minus 32 ce per path into it, with ce = min(c, lg - 1) for a tree of 2^lg leaves.  cap_log = 0: what zk_proof_data_len_stop
 * returns.  0 where that returns 0, or for cap_log > 8. */
size_t zk_proof_data_len_cap(uint32_t log_n, uint32_t log_blowup, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log,
                             int coset_leaves, uint32_t stop_log, uint32_t cap_log);
/* Proofs with challenges in the quadratic extension E (ext_log = 1; zk_ext_*): zk_proof_data_len_cap of the other arguments
 * with 24 bytes of alphas for 12, 8 per beta for 4, twice the bytes of the free term or of the coefficients, and 4 more bytes per value of cp
 * or of a FRI layer opened (the three f values of a query are unchanged).  ext_log = 0: what zk_proof_data_len_cap returns.  0 where that
 * returns 0, or for ext_log > 1 (2, the quartic extension, is reserved). */
size_t zk_proof_data_len_ext(uint32_t log_n, uint32_t log_blowup, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log,
                             int coset_leaves, uint32_t stop_log, uint32_t cap_log, uint32_t ext_log);
/* Shared proofs of M = 2^log_batch statements (zk_batch_prove_shared): zk_proof_data_len_cap of the other arguments, plus
 * 32 (M - 1) 2^ce_f + 12 (M - 1) in the head and 3 (M - 1) (12 + 32 (L - ce_f)) per query, ce_f = min(c, L - 1).  log_batch = 0: what
 * zk_proof_data_len_cap returns.  0 where that returns 0, or for log_batch > 8. */
size_t zk_proof_data_len_shared(uint32_t log_n, uint32_t log_blowup, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log,
                                int coset_leaves, uint32_t stop_log, uint32_t cap_log, uint32_t log_batch);
/* Proof-of-work search (zk_ctx_set_grinding): the smallest nonce >= start whose SHA-256(state || le64(nonce)) begins with
 * grind_bits zero bits (0..32; 0 gives start), on the GPU (zk_grind) or on <= 16 host threads (zk_grind_host; threads is
 * clamped to 1..16).  Gives up with an error naming grind_bits after 2^44 nonces.  A zk_channel user grinds on
 * zk_channel_state and commits the 8 little-endian bytes with zk_channel_commit. */
int zk_grind(int device, const uint8_t state[32], uint32_t grind_bits, uint64_t start, uint64_t *nonce_out);
int zk_grind_host(const uint8_t state[32], uint32_t grind_bits, uint64_t start, uint32_t threads, uint64_t *nonce_out);
/* compute_root_from_path (merkle.rs:82-110), CPU. */
int zk_compute_root_from_path(uint32_t element, size_t index, const uint8_t *path, size_t path_len,
                              uint8_t out[32]);

int zk_compute_root_from_path_ex(uint32_t element, size_t index, const uint8_t *path, size_t path_len,
                                 uint8_t out[32], int hash_kind);
/* The same from the s = 1, 2, 4 or 8 slot values of coset leaf `leaf` (zk_ctx_set_coset_leaves); s = 1 is the call above. */
int zk_compute_root_from_coset(const uint32_t *values, uint32_t s, size_t leaf, const uint8_t *path, size_t path_len,
                               uint8_t out[32], int hash_kind);

/* ---- batched verification on the GPU (csrc/verify.hip) ---------------------------------------------------------------
 * The check number the CPU verifier stops at: 0 = accepted; otherwise the number zk_verify_queries names in its error
 * (-(1000+k) / -1999 transcript replay when state != NULL, then verify_proof's -1 .. -8, -(100+k), -(200+k), -(300+k), -(400+k)).
 * Returns ZK_OK if accepted, ZK_ERR_VERIFY if rejected (check_out set either way), ZK_ERR_INVALID on bad arguments. */
int zk_verify_check(const uint8_t *proof, size_t len, const uint8_t *state, uint32_t log_n, uint32_t log_blowup,
                    uint32_t public_last, int hash_kind, uint32_t n_queries, int32_t *check_out);
/* zk_verify_check for proofs made with zk_ctx_set_grinding(grind_bits).  Strict (state != NULL): the nonce's hash must begin with
 * grind_bits zero bits, else -1998 -- checked after the beta challenges and before the first query challenge, without advancing
 * the k of -(1000+k); ANY nonce that meets the bits is accepted.  Not strict: the 8 nonce bytes are skipped unchecked -- the query
 * raws are read from the proof, not derived (as the reference does), so the work would certify nothing there.  A proof whose
 * length does not match grind_bits is rejected (-1). */
int zk_verify_grind(const uint8_t *proof, size_t len, const uint8_t *state, uint32_t log_n, uint32_t log_blowup,
                    uint32_t public_last, int hash_kind, uint32_t n_queries, uint32_t grind_bits, int32_t *check_out);

/* zk_verify_grind for proofs made with zk_ctx_set_fold(fold_log) (proof.rs:101-148 widened): per group the 2^steps opened values
 * are folded down with the formula of proof.rs:110-113 and compared with the next group's first value (the free term after the
 * last).  Check numbers as zk_verify_grind with "k" read as the group index j: -(100+j) fold, -(200+j) path length, -(300+j) path
 * of the first value, -(400+j) first failing path of the others; the replay counts 3 + G + q challenges.  fold_log = 1 gives every
 * input the number zk_verify_grind gives it. */
int zk_verify_fold(const uint8_t *proof, size_t len, const uint8_t *state, uint32_t log_n, uint32_t log_blowup,
                   uint32_t public_last, int hash_kind, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log, int32_t *check_out);

/* zk_verify_fold for proofs made with zk_ctx_set_coset_leaves.  With rot = (x % len) / (len / s), value t of a group is slot
 * (rot + t) % s of its leaf; from there on the fold arithmetic and its comparison are zk_verify_fold's.  Check numbers: -2 compares the
 * recomputed cp0 with group 0's value 0, -3 covers the three f path lengths, -4..-6 the f paths, -(100+j) / -(200+j) / -(300+j) the fold,
 * the path length and the path of group j; -7 and -(400+j) do not occur.  The replay counts 3 + G + q challenges and commits per
 * query three f tuples and one tuple per group.  A plain proof is rejected by length (-1), as a coset proof is by zk_verify_fold. */
int zk_verify_coset(const uint8_t *proof, size_t len, const uint8_t *state, uint32_t log_n, uint32_t log_blowup,
                    uint32_t public_last, int hash_kind, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log, int32_t *check_out);

/* zk_verify_fold (coset_leaves = 0) / zk_verify_coset (coset_leaves != 0) for proofs made with zk_ctx_set_fri_stop(stop_log = D), over
 * the G' groups of log_n - D rounds.  The last group's comparison "folded value == free term" becomes "== p(x^(2^R'))": p is evaluated by
 * Horner from the 2^D coefficients, each reduced mod P on reading, as raw challenges are; it keeps the check number -(100 + (G' - 1)).
 * The strict replay counts 3 + G' + q challenges, commits the coefficients in one piece and checks the nonce after them.  A proof whose
 * length is not zk_proof_data_len_stop of the arguments is rejected with -1, strict or not, and so is a stop_log outside the limits.
 * Soundness: one coset per committed layer is tested per query as before; the final polynomial's degree bound holds by construction.
 * stop_log = 0 gives every input the number zk_verify_fold / zk_verify_coset gives it (the same code path).
 * Many proofs at once on the GPU: zk_verifier_set_fri_stop + zk_verifier_run. */
int zk_verify_stop(const uint8_t *proof, size_t len, const uint8_t *state, uint32_t log_n, uint32_t log_blowup, uint32_t public_last,
                   int hash_kind, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log, int coset_leaves, uint32_t stop_log,
                   int32_t *check_out);

/* zk_verify_stop for proofs made with zk_ctx_set_merkle_cap(cap_log = c), every hash.  Each root of the header is the tree's 2^ce digests,
 * each path has lg - ce digests (another count: -3 / -(200+j), as ever) and is compared with cap entry leaf >> (lg - ce); a path that does
 * not reach its entry gets the check number the same path gets for missing the root.  Not strict (state == NULL): only the entries a
 * path lands in are tested.  A changed entry that no path lands in is caught by the strict replay alone, which commits each cap in one
 * piece, with the number a changed root gets there (the first challenge after it).  With c > 0 a proof whose length is not
 * zk_proof_data_len_cap of the arguments is rejected with -1, strict or not; cap_log > 8 is ZK_ERR_INVALID.  cap_log = 0 gives every
 * input the number zk_verify_stop gives it (the same code path). */
int zk_verify_cap(const uint8_t *proof, size_t len, const uint8_t *state, uint32_t log_n, uint32_t log_blowup, uint32_t public_last,
                  int hash_kind, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log, int coset_leaves, uint32_t stop_log,
                  uint32_t cap_log, int32_t *check_out);

/* zk_verify_cap for proofs whose challenges, composition polynomial and FRI layers lie in E = F_P[u] / (u^2 - 5) (ext_log = 1; DESIGN.md 7j
 * fixes the format), hashes 0 and 1.  The check numbers are zk_verify_cap's, one for one; a comparison of values of E (-2, a group's fold
 * -(100+j), the last fold against the free term or the final polynomial) fails when either component differs; the strict replay counts
 * 6 + 2G + q challenges.  Anything that is not zk_proof_data_len_ext bytes long: -1, strict or not.  ext_log = 0 is zk_verify_cap (the same
 * code path); ext_log > 1, and ext_log = 1 with BLAKE2s (which has no row leaf), are ZK_ERR_INVALID with *check_out = -1.
 * The one-call prover makes such proofs with zk_ctx_set_ext(ctx, 1). */
int zk_verify_ext(const uint8_t *proof, size_t len, const uint8_t *state, uint32_t log_n, uint32_t log_blowup, uint32_t public_last,
                  int hash_kind, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log, int coset_leaves, uint32_t stop_log,
                  uint32_t cap_log, uint32_t ext_log, int32_t *check_out);

/* zk_verify_cap for a shared proof of M = 2^log_batch statements (zk_batch_prove_shared), hashes 0..2; public_last: M values.  The same
 * code as zk_verify_cap with the statements summed: -2 compares sum_p (alpha0_p p0_p + alpha1_p p1_p + alpha2_p p2_p) at x with the cp
 * value opened (coset leaves: group 0's value 0); -3 covers the 3M f path lengths and cp's; -4 / -5 / -6 the path of f_p(x) / f_p(gx) /
 * f_p(g^2 x) of the first failing tuple in wire order, each into its entry of statement p's cap; -7, -8 and -(100+j) on as ever.  A
 * proof whose length is not zk_proof_data_len_shared of the arguments: -1, strict or not.  The strict replay counts 3M + G + q
 * challenges in -(1000+k) and commits the f level in one piece.  log_batch outside 1..8: *check_out = -1 and ZK_ERR_INVALID. */
int zk_verify_shared(const uint8_t *proof, size_t len, const uint8_t *state, uint32_t log_n, uint32_t log_blowup,
                     const uint32_t *public_last, uint32_t log_batch, int hash_kind, uint32_t n_queries, uint32_t grind_bits,
                     uint32_t fold_log, int coset_leaves, uint32_t stop_log, uint32_t cap_log, int32_t *check_out);

/* A verifier for many proofs of one size (log_n, log_blowup: the sizes zk_verify_queries accepts).  It owns its streams and
 * device buffers (grown on demand) and a pinned staging buffer.  One verifier is used from one host thread at a time. */
typedef struct zk_verifier zk_verifier;
int zk_verifier_create(int device, uint32_t log_n, uint32_t log_blowup, zk_verifier **out);
int zk_verifier_destroy(zk_verifier *v);
int zk_verifier_set_queries(zk_verifier *v, uint32_t n_queries);   /* 1..64, as zk_verify_queries */
int zk_verifier_set_hash(zk_verifier *v, int hash_kind);
/* Proofs made with zk_ctx_set_grinding(grind_bits): checks_out as zk_verify_grind gives them (-1998 in strict mode). */
int zk_verifier_set_grinding(zk_verifier *v, uint32_t grind_bits);
/* Proofs made with zk_ctx_set_fold / zk_batch_set_fold(fold_log): fold_log 1..3, default 1, from the next zk_verifier_run on (a
 * verifier may change factor between runs; its buffers grow for the longer proofs).  checks_out as zk_verify_fold gives them:
 * the replay counts 3 + G + q challenges, and "k" in -(100+k) / -(300+k) / -(400+k) is the group index.  Out of range:
 * ZK_ERR_INVALID and the setting is unchanged.  zk_verifier_get_fold: the current fold_log, 0 for a null verifier.
 * Measured (profiles/verify_fold_bench.txt). */
int zk_verifier_set_fold(zk_verifier *v, uint32_t fold_log);
uint32_t zk_verifier_get_fold(const zk_verifier *v);
/* Proofs made with zk_ctx_set_coset_leaves: off by default, any non-zero `on` means on, from the next zk_verifier_run on; it
 * combines with every hash, query count, grinding and fold_log 1..3 (fold_log 1 with coset leaves is a format of its own: every
 * group has two slots and one path).  A run then takes zk_proof_data_len_coset(log_n, log_blowup, q, grind_bits, fold_log) bytes
 * per proof and checks_out[i] is what zk_verify_coset gives proof i, for EVERY input; a proof with one-value leaves is rejected
 * with the number zk_verify_coset gives those bytes, and a coset proof by a verifier with the option off likewise with
 * zk_verify_fold's.  A null verifier: ZK_ERR_INVALID.  zk_verifier_get_coset_leaves: 1 or 0, 0 for a null verifier.
 * Not timed yet. */
int zk_verifier_set_coset_leaves(zk_verifier *v, int on);
int zk_verifier_get_coset_leaves(const zk_verifier *v);
/* Proofs made with zk_ctx_set_fri_stop(stop_log = D): default 0, from the next zk_verifier_run on (a verifier may change D between
 * runs; its buffers follow the proof length); it combines with every hash, query count, grinding, fold_log and leaf format, and no
 * order between the setters is imposed.  Limits, against the verifier's own sizes: D = 0, or 1 <= D <= 8 with D <= log_n - 1 and
 * D + log_blowup <= 12; anything else is ZK_ERR_INVALID and the setting is unchanged.  A run then takes
 * zk_proof_data_len_stop(log_n, log_blowup, q, grind_bits, fold_log, coset_leaves, D) bytes per proof and checks_out[i] is what
 * zk_verify_stop gives proof i with the same arguments, for EVERY input, strict or not: raw coefficients >= P are reduced on reading
 * as on the CPU, and a proof of another D is rejected with the number zk_verify_stop gives those bytes.  With D = 0 lengths and
 * launches are what they were.  A null verifier: ZK_ERR_INVALID.  zk_verifier_get_fri_stop: the current D, 0 for a null verifier.
 * Not run or timed on a GPU yet (tools/verify_bench.py --stop is the tool; DESIGN.md 7d "Early stop"). */
int zk_verifier_set_fri_stop(zk_verifier *v, uint32_t stop_log);
uint32_t zk_verifier_get_fri_stop(const zk_verifier *v);
/* Proofs made with zk_ctx_set_merkle_cap(cap_log = c): default 0, 0 <= c <= 8 (anything else: ZK_ERR_INVALID, the setting unchanged), from
 * the next zk_verifier_run on; it combines with every fold_log, leaf format, stop_log, query count, grinding and both hashes of this
 * class.  zk_verifier_run then takes zk_proof_data_len_cap(log_n, log_blowup, q, grind_bits, fold_log, coset_leaves, D, c) bytes per proof
 * and checks_out[i] is what zk_verify_cap gives proof i with the same arguments, for EVERY input, strict or not: a path is hashed
 * lg - ce times and compared with the cap entry it lands in, the strict replay commits each cap in one piece, a proof of another cap is
 * rejected with the number zk_verify_cap gives those bytes, and proofs whose path counts differ from the fixed layout go to the CPU
 * verifier with c.  Kernels of their own read the per-tree layout from a table in the launch arguments (csrc/verify.hip); with c = 0
 * lengths, results and launches are what they were.  zk_verifier_get_merkle_cap: the current c, 0 for a null verifier. */
int zk_verifier_set_merkle_cap(zk_verifier *v, uint32_t cap_log);
uint32_t zk_verifier_get_merkle_cap(const zk_verifier *v);
/* Shared proofs made with zk_batch_prove_shared (log_batch = lb: ONE proof of M = 2^lb statements), with or without row leaves
 * (zk_batch_set_shared_rows): lb 0..8, default 0 = plain proofs; row_leaves (any non-zero value: on) needs lb >= 1.  An lb out of
 * range, row leaves with lb 0 or a null verifier: ZK_ERR_INVALID and the setting unchanged.  From the next zk_verifier_run on (a verifier
 * may change it between runs); it combines with every query count, grinding, fold_log, leaf format, stop_log, cap_log and both hashes of
 * this class.  zk_verifier_run then takes zk_proof_data_len_shared_rows(log_n, log_blowup, q, grind_bits, fold_log, coset_leaves, D, c,
 * lb, row_leaves) bytes per proof and public_last[count][M], statement-major per proof, and checks_out[i] is what zk_verify_shared_rows
 * gives proof i with the same arguments, for EVERY input, strict or not.  Kernels of their own (csrc/verify.hip "shared proofs"): the
 * -2 relation is summed over the statements on one lane per (proof, query); the f paths run one lane per (proof, statement), or with row
 * leaves one lane per proof, each row hashed as zk_row_leaf_hash hashes it; the strict replay is one lane per proof.  Proofs whose path
 * counts differ from the fixed layout go to the CPU verifier with their M public values.  With lb = 0 lengths, results and launches are
 * what they were.  zk_verifier_get_shared: the current lb, 0 for a null verifier; zk_verifier_get_shared_rows: 1 or 0, 0 for a null
 * verifier. */
int zk_verifier_set_shared(zk_verifier *v, uint32_t log_batch, int row_leaves);
uint32_t zk_verifier_get_shared(const zk_verifier *v);
int zk_verifier_get_shared_rows(const zk_verifier *v);
/* Proofs made with zk_ctx_set_ext(ext_log = 1), challenges, cp and FRI layers in E = F_P[u] / (u^2 - 5): ext_log 0
 * (default) or 1, from the next zk_verifier_run on (a verifier may change it between runs); it combines with every fold_log, leaf
 * format, stop_log, cap_log, query count, grinding and both hashes of this class.  zk_verifier_run then takes
 * zk_proof_data_len_ext(log_n, log_blowup, q, grind_bits, fold_log, coset_leaves, D, c, 1) bytes and one public value per proof, and
 * checks_out[i] is what zk_verify_ext gives proof i with the same arguments, for EVERY input, strict or not.  Kernels of their own
 * (csrc/verify.hip "proofs over E"): both components of every comparison, row leaves of the values' words, two draws per challenge in the
 * strict replay; proofs whose path counts differ from the fixed layout go to the CPU verifier.  A null verifier or ext_log > 1:
 * ZK_ERR_INVALID and the setting unchanged.  Ext and shared proofs refuse each other, whichever is set second: zk_verifier_set_ext(v, 1)
 * on a verifier with log_batch >= 1, and zk_verifier_set_shared(v, lb >= 1, .) on one with ext on, are ZK_ERR_INVALID and change nothing.
 * With ext_log = 0 lengths, results and launches are what they were.  zk_verifier_get_ext: the current ext_log, 0 for a null verifier. */
int zk_verifier_set_ext(zk_verifier *v, uint32_t ext_log);
uint32_t zk_verifier_get_ext(const zk_verifier *v);
/* count proofs at proofs + i*stride, each exactly zk_proof_data_len_fold(log_n, log_blowup, q, grind_bits, fold_log) bytes (with
 * the defaults zk_proof_data_len_queries(log_n, log_blowup, q); with coset leaves zk_proof_data_len_coset of the same arguments;
 * with an early stop zk_proof_data_len_stop; stride >= that, any alignment); states: count*32 bytes, or NULL = not strict;
 * public_last[count].  checks_out[i] = what zk_verify_fold (fold_log 1: zk_verify_grind, zk_verify_check; coset leaves:
 * zk_verify_coset; an early stop: zk_verify_stop) returns in check_out for proof i,
 * for EVERY input.  Returns ZK_OK if all were accepted, ZK_ERR_VERIFY if any was rejected
 * (zk_last_error names the first rejected index and its check), other errors as usual.  count = 0 is a no-op. */
int zk_verifier_run(zk_verifier *v, const uint8_t *proofs, size_t stride, size_t count, const uint8_t *states,
                    const uint32_t *public_last, int32_t *checks_out);

/* ---- Channel (channel.rs:6-37), host only ------------------------------------ */
int zk_channel_new(zk_channel **out);                                        /* channel.rs:12 */
int zk_channel_free(zk_channel *ch);
/* Adopts the two fields of a Channel kept on the caller's side (channel.rs:6-9: state, data): how the reference's
 * Rust Channel argument of generate_proof (prover.rs:9) crosses the FFI; read back with zk_channel_state / _data. */
int zk_channel_import(zk_channel *ch, const uint8_t state[32], const uint8_t *data, size_t n);
int zk_channel_commit(zk_channel *ch, const uint8_t *bytes, size_t n);       /* channel.rs:19 */
int zk_channel_get_u32(zk_channel *ch, uint32_t *out);                       /* channel.rs:28 */
int zk_channel_state(const zk_channel *ch, uint8_t out[32]);
size_t zk_channel_data_len(const zk_channel *ch);
int zk_channel_data(const zk_channel *ch, uint8_t *out, size_t cap);         /* channel.rs:34 */

/* FRI tail: the last layers of a proof whose earlier layers live elsewhere (one proof sharded over
 * several GPUs hands over once a layer is small enough to be replicated).  Layer rho0 of a
 * (log_n, log_blowup) proof is layer 0 of a domain with log_n_tail = log_n - rho0 and shift
 * w^(2^rho0).  zk_tail_run copies the handed-over layer (2^(log_n_tail+log_blowup) words at d_layer0,
 * produced on src_stream), commits it, then runs the remaining log_n_tail rounds of prover.rs:198-225
 * (fused fold + commit) on the caller's channel: betas_out[log_n_tail], roots_out[(log_n_tail+1)*32].
 * zk_tail_open gathers the openings of prover.rs:280-289 for the tail layers.  Destroy with
 * zk_ctx_destroy. */
int zk_tail_create(int device, uint32_t log_n_tail, uint32_t log_blowup, uint32_t shift, zk_ctx **out);
int zk_tail_run(zk_ctx *tail, const uint32_t *d_layer0, void *src_stream, zk_channel *ch, int hash_kind,
                uint32_t *betas_out, uint8_t *roots_out, uint32_t *free_term_out);
int zk_tail_open(zk_ctx *tail, size_t x, uint32_t *vals_out, uint8_t *paths_out);

/* ---- one proof sharded over the GPUs of one node (BASELINE.json configs[3]) ----------------
 * generate_proof (prover.rs:9-293) with the evaluation domain distributed CYCLICALLY over `world` ranks, one process
 * (or thread) per GPU: rank r holds the elements i = r (mod world) of every layer, which is again a coset domain, so
 * LDE, composition and every fold run the single-GPU kernels with no communication.  The only exchange is the
 * commitment: one all-to-all per committed layer turns the cyclic layout into contiguous leaf blocks (the transpose
 * of a four-step NTT over the ranks), each rank hashes its subtree, the `world` subtree roots are exchanged and the
 * top log2(world) levels are hashed on the host.  Layers below 2^21 values (2^20 from 4 ranks on) are replicated and finished by every rank
 * (zk_tail_*).  Every rank runs the same transcript and returns the same proof bytes, identical to zk_prove's.
 *
 * Transport.  By default the collectives are RCCL's (librccl.so.1 is loaded at run time; grouped ncclSend/ncclRecv for
 * the all-to-all, ncclAllGather): rank 0 calls zk_shard_unique_id, the caller distributes the 128 bytes (any side
 * channel: MPI, a file, torch.distributed) and every rank passes them to zk_shard_create.  A caller that owns its own
 * communication passes a zk_shard_transport instead (device pointers, stream-ordered on `stream`); tests use that to
 * run several ranks on one GPU.  world must be a power of two dividing the blow-up. */
typedef struct zk_shard zk_shard;
#define ZK_SHARD_ID_BYTES 128
typedef struct zk_shard_transport {
    void *user;
    /* send[p] (words u32) goes to rank p, recv[q] (words u32) comes from rank q; p, q < world, own part included */
    int (*all_to_all)(void *user, const uint32_t *const *send, uint32_t *const *recv, size_t words, void *stream);
    /* recv[q * words ..] = rank q's send */
    int (*all_gather)(void *user, const uint32_t *send, uint32_t *recv, size_t words, void *stream);
} zk_shard_transport;
typedef struct zk_shard_options {   /* zero = default (struct_size excepted) */
    uint32_t struct_size;       /* sizeof(zk_shard_options), set by the caller (see "ABI version" above) */
    uint32_t min_layer_log;     /* a FRI layer stays sharded while it has >= 2^this values in total (21; 20 from 4 ranks on) */
    uint32_t min_chunk_log;     /* ... and >= 2^this leaves per (rank, peer) piece (14) */
    uint32_t overlap_min_log;   /* pieces of >= 2^this words are exchanged in 4 chunks overlapped with the hashing (21) */
    int force_collectives;      /* run the collectives even with world = 1 (exercises the transport on one GPU) */
    int no_root_board;          /* exchange subtree roots with an all-gather instead of the shared-memory board */
    int plain_collectives;      /* no chunked exchange and no shared-memory roots: one all-to-all per layer on the main
                                   stream, subtree roots by all-gather (the fall-back rung of bench.py --gpus N) */
    int single_build_stream;    /* chunk builds of a layer on one stream (A/B; default: two alternating streams) */
    int single_communicator;    /* built-in RCCL transport: the exchange stream shares the main communicator (default: the
                                   chunked exchanges get a communicator of their own, see below) */
    int exchange_cp;            /* 1: commit cp by exchanging it like every other layer (what rounds 1-4 did; A/B).  Default:
                                   cp over a rank's block is recomputed from the block of f the rank received for the
                                   commitment of f, inside the leaf hashing -- no exchange for cp (zk_shard_plan_info.cp_from_f) */
    double timeout_s;           /* bound of every host-side wait on a peer; 0 = environment ZK_SHARD_TIMEOUT_S, else 120 s */
    int peer_copy;              /* transport == NULL: instead of RCCL, the built-in PEER-COPY transport (csrc/peer.hpp): every rank of
                                   the node publishes the IPC handle of ONE staging buffer on a shared-memory page at creation, a
                                   collective copies its pieces there and every rank pulls its piece with a device-to-device copy.
                                   Host-synchronous (implies plain_collectives); `id` is any 128 bytes shared by the ranks.  The rung
                                   below "RCCL, plain collectives": for a node where no communicator can be formed (bench.py --gpus N
                                   falls back to it) */
    int reserved;
} zk_shard_options;
typedef struct zk_shard_stats {
    uint32_t struct_size;       /* sizeof(zk_shard_stats), set by the caller (see "ABI version" above) */
    uint32_t sharded_layers;    /* FRI layers 0 .. sharded_layers-1 (and f) are distributed; the rest is the replicated tail */
    uint32_t root_board;        /* 1: subtree roots travel through shared memory (all ranks on one node) */
    uint32_t chunked_layers;    /* layers of the last proof exchanged in chunks overlapped with the hashing */
    uint32_t native_rccl;       /* 1: the built-in RCCL transport */
    uint32_t rccl_nranks;       /* ncclCommCount of the communicator (checked against `world` at creation); 0 without RCCL */
    uint32_t communicators;     /* RCCL communicators in use: 2 when the chunked exchanges have their own, else 1; 0 without RCCL */
    double sent_bytes;          /* bytes this rank sent to OTHER ranks during the last zk_shard_prove* / lde_commit */
    double all_to_all_bytes;    /* ... of which in the per-commitment all-to-alls */
    double setup_ms;
    double device_bytes;
    /* zk_shard_set_profiling(s, 1): HIP events around the exchanges of the last zk_shard_prove* / lde_commit (0 otherwise).
     * exchange_ms: summed durations of the all-to-alls and all-gathers on their streams (for a chunked layer this includes
     * the time the exchange kernel waits for compute units beside the hashing); exposed_exchange_ms: the part of it the
     * hashing streams spent stalled (a plain exchange is exposed in full, a chunk only while its build waits for it);
     * tail_ms: host time of the replicated tail (all-gather of the first replicated layer, then zk_tail_run);
     * decommit_ms: host time from the query index to the last opening in the channel; selftest_ms: the known-pattern
     * exchange run by zk_shard_create. */
    double exchange_ms;
    double exposed_exchange_ms;
    double tail_ms;
    double selftest_ms;
    double decommit_ms;         /* host time of the decommitment (prover.rs:266-289), all queries, profiling on */
    uint32_t exchanges;         /* collectives timed (profiling on) */
    uint32_t selftest_ok;       /* 1: zk_shard_create's known-pattern all-to-all + all-gather arrived in the right places */
    uint32_t peer_copy;         /* 1: the built-in peer-copy transport (zk_shard_options.peer_copy) */
    uint32_t reserved;
} zk_shard_stats;
/* The layout of a sharded proof, as a pure function of its arguments (no GPU, no communication): what
 * zk_shard_create will do.  Layer ids: 0 = f_eval, 1 + r = FRI layer r. */
typedef struct zk_shard_plan_info {
    uint32_t struct_size;        /* sizeof(zk_shard_plan_info), set by the caller (see "ABI version" above) */
    uint32_t world;
    uint32_t log_world;
    uint32_t sharded_layers;     /* FRI layers 0 .. sharded_layers-1 (and f) are distributed */
    uint32_t tail_rounds;        /* FRI rounds of the replicated tail */
    uint32_t chunked_layers;     /* committed layers exchanged in chunks overlapped with the hashing */
    uint32_t chunked_mask;       /* bit id set: layer id is exchanged in chunks */
    uint32_t log_chunks;         /* a chunked layer is exchanged in 2^log_chunks chunks */
    uint32_t min_layer_log;      /* the thresholds in force (options and defaults; plain_collectives: overlap_min_log = 99) */
    uint32_t min_chunk_log;
    uint32_t overlap_min_log;
    uint32_t piece_log[32];      /* log2 words of one (rank, peer) piece of layer id */
    double all_to_all_bytes;     /* bytes one rank sends to its peers in the all-to-alls of one proof */
    double lde_commit_bytes;     /* ... of zk_shard_lde_commit (layer 0 only) */
    uint32_t cp_from_f;          /* 1: cp (layer id 1) is committed without an exchange: recomputed over the rank's block from the
                                    received block of f plus a 2B-word all-gather (the positions after the block); its piece
                                    is then not part of all_to_all_bytes */
    uint32_t reserved;
} zk_shard_plan_info;
int zk_shard_plan(int world, uint32_t log_n, uint32_t log_blowup, const zk_shard_options *opt, zk_shard_plan_info *out);
/* Streams and communicators.  Plain exchanges run on the prover's main stream.  Chunked exchanges (pieces of >=
 * 2^overlap_min_log words) run on a second, high-priority stream beside the hashing; with the built-in transport they use a
 * second RCCL communicator created for that stream (rank 0 draws its id and the first communicator distributes it), so no
 * communicator is ever driven from two streams, and every collective additionally waits (HIP event) for the previous
 * collective of the other stream, so no ordering rests on RCCL's internal serialisation.  A caller transport is called
 * with either stream and must tolerate that.
 * zk_shard_create ends with a self-test when collectives are in use: an all-to-all (on each stream in use) and an
 * all-gather (on the main stream, and on the exchange stream when the halo of cp travels there) of a known pattern, the
 * all-to-all at the size of the largest piece; every word must arrive at its place, else the call
 * fails with ZK_ERR_HIP naming the first wrong (peer, word).  It also brings RCCL's lazy connections up before the
 * first proof.  zk_shard_self_test repeats it on request.
 * ncclCommInitRank itself is not bounded by this library (it cannot be cancelled): a caller that must not hang runs
 * its ranks under a watchdog (bench.py does).
 *
 * ncclGetUniqueId through the same run-time loaded RCCL (rank 0, before zk_shard_create). */
int zk_shard_unique_id(uint8_t id_out[ZK_SHARD_ID_BYTES]);
/* Collective over the `world` ranks (ncclCommInitRank when transport is NULL).  id: the shared 128 bytes; with a
 * caller transport they only name the shared-memory root board (NULL: no board).  opt may be NULL. */
int zk_shard_create(int device, int rank, int world, const uint8_t *id, const zk_shard_transport *transport,
                    const zk_shard_options *opt, uint32_t log_n, uint32_t log_blowup, zk_shard **out);
int zk_shard_destroy(zk_shard *s);
/* The same n-1 trace values on every rank (prover.rs:32-39; the interpolant is replicated). */
int zk_shard_trace_upload(zk_shard *s, const uint32_t *trace, size_t count);
/* generate_proof on the caller's channel (prover.rs:9), collectively; every rank gets the same transcript. */
int zk_shard_prove_channel(zk_shard *s, zk_channel *ch);
int zk_shard_prove(zk_shard *s, uint8_t *proof_out, size_t cap, size_t *proof_len, uint8_t state_out[32]);
/* configs[3] shape: sharded LDE, all-to-all transpose, Merkle commit; root of f_eval (prover.rs:60-85). */
int zk_shard_lde_commit(zk_shard *s, uint8_t root_out[32]);
/* Merkle hash (zk_hash_kind) and number of decommitment queries, as zk_ctx_set_hash / zk_ctx_set_queries; every rank
 * must use the same values.  Verify with zk_verify_queries(..., hash_kind, n_queries). */
int zk_shard_set_hash(zk_shard *s, int hash_kind);
int zk_shard_set_queries(zk_shard *s, uint32_t n_queries);
/* Failure handling.  A rank that leaves zk_shard_prove* / zk_shard_lde_commit with an error posts an abort on the shared
 * root board (peers waiting for it return ZK_ERR_HIP naming this rank instead of waiting out zk_shard_options.timeout_s),
 * refuses further proofs, and zk_shard_destroy then aborts its RCCL communicators (ncclCommAbort).  The board's abort
 * words are mapped whenever the ranks share a node, also when the roots themselves travel by all-gather
 * (no_root_board, plain_collectives).  With a caller transport nothing can abort a collective that is already
 * enqueued: zk_shard_destroy of a failed prover then does not wait for its streams (they are leaked with a message).
 * zk_shard_inject_failure makes a rank fail that way on purpose (tests). */
int zk_shard_inject_failure(zk_shard *s, int code);
/* Known-pattern all-to-all + all-gather through the prover's transport (collective; see above).  The pattern is written into
 * the storage of layer 0 (f_eval) and the receive buffer: the layers resident from an earlier zk_shard_prove* / _lde_commit are
 * INVALID afterwards (zk_shard_layer_read(0, ..) would return pattern words) until the next proof recomputes them. */
int zk_shard_self_test(zk_shard *s);
/* on != 0: time the exchanges of later proofs with HIP events (zk_shard_stats.exchange_ms ...); costs a few event
 * records per layer, so benchmarks switch it on for one untimed proof. */
int zk_shard_set_profiling(zk_shard *s, int on);
int zk_shard_last_transcript(const zk_shard *s, zk_transcript_info *out);
/* This rank's shard of a layer (0 = f_eval, 1 + r = FRI layer r < sharded_layers): element j is global index
 * rank + world * j. */
int zk_shard_layer_read(zk_shard *s, uint32_t layer, size_t offset, size_t count, uint32_t *out);
int zk_shard_get_stats(const zk_shard *s, zk_shard_stats *out);

/* Timing of the zk_dev_* launches (process-wide; same classes and semantics as
 * zk_ctx_set_profiling / zk_kernel_stats). */
int zk_dev_set_profiling(uint32_t class_mask);
int zk_dev_kernel_stats(zk_kernel_stat *out, size_t count, int reset);

/* Roofline probe (measurement only; bench.py `roofline.valu.chain_*`): every lane of waves_per_simd resident waves per
 * SIMD runs a dependent chain of `hashes` inner hashes (merkle.rs:42-45 shape) with no memory traffic, `launches`
 * launches back to back.  ns_per_hash_per_simd is the steady-state time one SIMD needs per hash of one wave; divided
 * by the hash's VALU instruction count it is the issue rate the Merkle kernels can reach at best at that residency. */
typedef struct zk_chain_probe {
    uint32_t struct_size;          /* sizeof(zk_chain_probe), set by the caller (see "ABI version" above) */
    uint32_t reserved;
    double ns_per_hash_per_simd;
    double clock_ghz;              /* median over the waves: shader clocks per 100 MHz reference tick */
    double ms;                     /* wall time of the timed launches (HIP events) */
    uint32_t waves_per_simd;
    uint32_t launches;
    uint32_t hashes;
    uint32_t cus;                  /* compute units of the device */
} zk_chain_probe;
int zk_probe_hash_chain(int device, int hash_kind, uint32_t waves_per_simd, uint32_t hashes, uint32_t launches, zk_chain_probe *out);

/* Test hook (configs[4]): the field hash exists in several forms on the device -- double precision one lane per node (every tree is
 * built with it, csrc/fieldhash_f64.hpp), its quad and 16-lane row forms (the narrow tree levels), 32-bit Montgomery (the host's form:
 * verifier, tree tops of the sharded prover) and the 32-bit row form of rounds 3-4.  Hashes `count` pseudo-random inputs, every 16th an edge pattern (words 0, P - 1, raw words >= P), through
 * all of them: *mismatches = inputs on which they differ or a digest word is not canonical (must be 0). */
int zk_probe_fieldhash_forms(int device, uint32_t count, uint32_t seed, uint32_t *mismatches, uint32_t *first_bad);

/* ---- stand-alone primitives on host buffers (upload, run on the GPU, download) -- */
/* Merkle::new(size, data) (merkle.rs:14): nodes_out = (2m-1)*32 bytes, heap order. */
int zk_merkle_build_host(int device, const uint32_t *vals, size_t m, uint8_t *nodes_out);
int zk_merkle_build_host_ex(int device, const uint32_t *vals, size_t m, uint8_t *nodes_out, int hash_kind);
/* Natural-order NTT / inverse NTT of size 2^log_m with the canonical root
 * zk_field_root_of_unity(log_m); in place on the host buffer. */
int zk_ntt_host(int device, uint32_t *data, uint32_t log_m, int inverse);
/* trace (n-1 values) -> N coset evaluations (same as zk_trace_upload + zk_lde + read). */
int zk_lde_host(int device, const uint32_t *trace, uint32_t log_n, uint32_t log_blowup, uint32_t *out);

/* ---- coset domains and device-pointer primitives (stream-ordered) ------------------
 * For callers that own the device buffers and the orchestration (the sharded prover, csrc/shard.hip,
 * drives these between RCCL collectives).  A domain is
 * {shift * h^i, i < 2^(log_n+log_blowup)}, h = zk_field_root_of_unity(log_n+log_blowup), with
 * the tables the kernels need; the reference's domain is shift = 5 (prover.rs:69).  log_blowup
 * may be 0.  fold_only != 0 builds only what zk_dev_fri_fold needs.  Entry points that take only device
 * pointers and a stream (zk_dev_merkle_build*, zk_dev_interleave, zk_dev_gather, ...) launch on the
 * calling thread's current device: select the device the buffers live on first (hipSetDevice /
 * torch.cuda.set_device), as one process per GPU does once at start-up. */
typedef struct zk_dom zk_dom;
int zk_dom_create(int device, uint32_t log_n, uint32_t log_blowup, uint32_t shift, int fold_only, zk_dom **out);
int zk_dom_destroy(zk_dom *dom);
/* lagrange + solve (polynomial.rs:337, :49; prover.rs:60-70).  d_trace: n words = a[0..n-2] followed
 * by 0; d_coef: 2n words scratch; d_out: N words, natural order. */
int zk_dev_lde(const zk_dom *dom, const uint32_t *d_trace, uint32_t *d_coef, uint32_t *d_out, void *stream);
/* prover.rs:101-173 pointwise; first = a[0], last = a[n-2]. */
int zk_dev_compose(const zk_dom *dom, const uint32_t *d_f, uint32_t *d_cp, uint32_t first, uint32_t last,
                   const uint32_t alpha_raw[3], void *stream);
/* polynomial.rs:385 + prover.rs:204-211: 2^log_m values of FRI layer `round` -> 2^(log_m-1). */
int zk_dev_fri_fold(const zk_dom *dom, const uint32_t *d_in, uint32_t *d_out, uint32_t log_m, uint32_t round,
                    uint32_t beta_raw, void *stream);
/* The same `steps` (1..3) times in one pass with the challenges beta, beta^2, beta^4: 2^log_m values of FRI layer `round` ->
 * 2^(log_m-steps) values of layer round + steps (round + steps <= log_n).  steps = 1 is zk_dev_fri_fold. */
int zk_dev_fri_fold_multi(const zk_dom *dom, const uint32_t *d_in, uint32_t *d_out, uint32_t log_m, uint32_t round,
                          uint32_t steps, uint32_t beta_raw, void *stream);
/* The composition and the group fold with challenges in E = F_P[u] / (u^2 - 5) (zk_ext_*).  A layer of len values of
 * E is two planes: component 0 at words [0, len), component 1 at [len, 2 len); f stays in the base field.
 * zk_dev_compose_ext: alpha_raw = alpha0.c0, alpha0.c1, alpha1.c0, alpha1.c1, alpha2.c0, alpha2.c1 (raws, reduced mod P); d_cp takes
 * 2 N words, and plane j is what zk_dev_compose gives with (alpha0.cj, alpha1.cj, alpha2.cj) -- in one pass over f.
 * zk_dev_fri_fold_multi_ext: d_in = 2 * 2^log_m words, d_out = 2 * 2^(log_m-steps); beta_raw = (c0, c1), the challenges beta,
 * beta^2, beta^4 squared in E; steps = 1..3.  With beta_raw[1] = 0 each plane is zk_dev_fri_fold_multi of that plane.
 * The one-call prover runs them with zk_ctx_set_ext(ctx, 1) (the batched prover has forms of its own, zk_dev_*_ext_batch below); the
 * stage-by-stage context API and the sharded prover are base-field; zk_verify_ext is the CPU verifier of the format. */
int zk_dev_compose_ext(const zk_dom *dom, const uint32_t *d_f, uint32_t *d_cp, uint32_t first, uint32_t last,
                       const uint32_t alpha_raw[6], void *stream);
int zk_dev_fri_fold_multi_ext(const zk_dom *dom, const uint32_t *d_in, uint32_t *d_out, uint32_t log_m, uint32_t round,
                              uint32_t steps, const uint32_t beta_raw[2], void *stream);
/* zk_dev_fri_fold_multi over a proof-major batch: d_in = [batch][2^log_m], d_out = [batch][2^(log_m-steps)], proof b folded with
 * its own challenge d_beta_raw[b] (raw u32 values on the device; values >= P are accepted and reduced).  d_work: 8 * batch words of
 * caller scratch for the per-proof constants.  Stream-ordered: two launches, no allocation, no host synchronisation.  Any
 * batch >= 1 with batch * 2^log_m <= 2^32; batch = 1 gives what zk_dev_fri_fold_multi gives. */
int zk_dev_fri_fold_multi_batch(const zk_dom *dom, const uint32_t *d_in, uint32_t *d_out, uint32_t log_m, uint32_t round,
                                uint32_t steps, const uint32_t *d_beta_raw, uint32_t *d_work, uint32_t batch, void *stream);
/* The kernels of the batched prover over E (zk_batch_set_ext).  A layer of E of a batch is two planes, component 0 first,
 * each proof-major: value i of proof b at words b * len + i and batch * len + b * len + i.  Stream-ordered, no allocation.
 * zk_dev_compose_ext_batch: d_f = [batch][N], d_cp = two planes [batch][N]; first, last ([batch]) and alpha_raw ([batch][6], in
 * zk_dev_compose_ext's order) are HOST arrays, turned into the per-proof tables in d_work (12 * batch words, 16-byte aligned; the
 * call waits for that copy, then launches).  Plane j of proof b is zk_dev_compose of proof b's f with component j of its alphas.
 * zk_dev_fri_fold_multi_ext_batch: d_in = two planes [batch][2^log_m], d_out = two planes [batch][2^(log_m-steps)], proof b folded with
 * the challenge (d_beta_raw[2 b], d_beta_raw[2 b + 1]) (raw u32 values on the device; values >= P are accepted and reduced).  d_work:
 * 24 * batch words of scratch, 16-byte aligned.  Two launches.  Proof b's planes are zk_dev_fri_fold_multi_ext of its input planes.
 * zk_dev_merkle_build_coset_ext_batch: d_vals = two planes [2^log_batch][2^log_len], steps 1..3 < log_len, hash 0 or 1; d_nodes: the
 * heap over 2^(log_batch + log_len - steps) leaves, all (2 leaves - 1) * 8 words, leaf (p, c) the row leaf (zk_row_leaf_hash) of the
 * 2 * 2^steps words d_vals[plane * batch * len + p * len + c + u * (len >> steps)], component 0's slots first.
 * Any batch >= 1 with batch * 2^log_m <= 2^32 for the first two. */
int zk_dev_compose_ext_batch(const zk_dom *dom, const uint32_t *d_f, uint32_t *d_cp, const uint32_t *first, const uint32_t *last,
                             const uint32_t *alpha_raw, uint32_t *d_work, uint32_t batch, void *stream);
int zk_dev_fri_fold_multi_ext_batch(const zk_dom *dom, const uint32_t *d_in, uint32_t *d_out, uint32_t log_m, uint32_t round,
                                    uint32_t steps, const uint32_t *d_beta_raw, uint32_t *d_work, uint32_t batch, void *stream);
int zk_dev_merkle_build_coset_ext_batch(const uint32_t *d_vals, uint32_t log_len, uint32_t steps, uint32_t log_batch, uint32_t *d_nodes,
                                        void *stream, int hash_kind);
/* Batch trace generation: prover.rs:32-39 is serial per trace, so one
 * lane generates one trace; out[t*count + i] = a_i of trace t seeded by (a0[t], a1[t]). */
int zk_dev_trace_fibsq_batch(const uint32_t *d_a0, const uint32_t *d_a1, uint32_t batch, uint32_t count,
                             uint32_t *d_out, void *stream);
int zk_trace_fibsq_batch_host(int device, const uint32_t *a0, const uint32_t *a1, uint32_t batch,
                              uint32_t count, uint32_t *out);
/* out[u * parts + q] = in[q * cnt + u]: cyclic <-> block layout around the all-to-all. */
int zk_dev_interleave(const uint32_t *d_in, uint32_t *d_out, uint32_t log_parts, uint32_t log_cnt, void *stream);
/* d_out[i*words ..] = d_src[d_offsets[i] .. + words]. */
int zk_dev_gather(const uint32_t *d_src, const uint64_t *d_offsets, uint32_t count, uint32_t words,
                  uint32_t *d_out, void *stream);
/* d_vals: m u32 on the device; d_nodes: (2m-1)*8 u32 state words, heap order. */
int zk_dev_merkle_build(const uint32_t *d_vals, uint32_t log_m, uint32_t *d_nodes, void *stream);
int zk_dev_merkle_build_ex(const uint32_t *d_vals, uint32_t log_m, uint32_t *d_nodes, void *stream, int hash_kind);
/* Same tree, with the leaves still in all-to-all order: 2^log_parts pieces of 2^log_cnt words, leaf
 * u*parts + q = d_recv[q*cnt + u] (zk_dev_interleave fused into the leaf hashing). */
int zk_dev_merkle_build_interleaved(const uint32_t *d_recv, uint32_t log_parts, uint32_t log_cnt,
                                    uint32_t *d_nodes, void *stream, int hash_kind);
/* Commitment with the root handed to the host (what prover.rs:85 feeds the channel): the tree of
 * zk_dev_merkle_build_ex (log_parts = 0, d_src in natural order) or zk_dev_merkle_build_interleaved
 * (log_parts > 0).  With SHA-256 and SHA extensions on the CPU the device stops at depth 8, the calling
 * thread hashes the 255 nodes above (see zk_ctx_set_host_levels) and a copy ordered on `stream` completes
 * d_nodes; the call returns once the root is known.  One committer per host thread;
 * consecutive commits may use different streams (the staging buffer of the previous commit is released by an event). */
typedef struct zk_committer zk_committer;
int zk_committer_create(int device, zk_committer **out);
int zk_committer_destroy(zk_committer *k);
/* Hand-over depth of later commits (top_log of zk_ctx_set_host_levels; <= 8; 0 = the device builds to the root). */
int zk_committer_set_top(zk_committer *k, uint32_t top_log);
int zk_dev_merkle_commit(zk_committer *k, const uint32_t *d_src, uint32_t log_parts, uint32_t log_cnt,
                         uint32_t *d_nodes, void *stream, int hash_kind, uint8_t root_out[32]);
/* zk_dev_merkle_finish with the same hand-over: for a tree built with zk_dev_merkle_build_chunk. */
int zk_dev_merkle_commit_finish(zk_committer *k, uint32_t *d_nodes, uint32_t log_m, uint32_t log_chunks,
                                void *stream, int hash_kind, uint8_t root_out[32]);
/* The same tree in 2^c aligned chunks, so that hashing chunk i overlaps the exchange of chunk i+1: chunk
 * `chunk` covers leaves [chunk << s, (chunk+1) << s), s = log_parts + log_cnt, arriving in its own
 * receive buffer in all-to-all order; the throughput-bound levels are built in place in the heap over
 * 2^log_m leaves.  zk_dev_merkle_finish then runs the latency-bound top of the whole tree once. */
int zk_dev_merkle_build_chunk(const uint32_t *d_recv, uint32_t log_parts, uint32_t log_cnt, uint32_t *d_nodes,
                              uint32_t log_m, uint32_t chunk, void *stream, int hash_kind);
int zk_dev_merkle_finish(uint32_t *d_nodes, uint32_t log_m, uint32_t log_chunks, void *stream, int hash_kind);
/* Tuning / test hook, process-wide: a Merkle build runs throughput launches (a wave owns 64 * 2^k leaves) while a level
 * has more than 2^log_nodes nodes and finishes the tree in workgroup-local launches below that (default 17: measured
 * flat between 16 and 18; 0 restores the default; 12 .. 24).  Results do not depend on it; tests lower it to drive
 * small trees through the chunked build (zk_dev_merkle_build_chunk / _finish).  Call it while no build is in flight. */
int zk_dev_set_merkle_latency_log(uint32_t log_nodes);
/* Byte view of nodes stored as state words: out[32] for node `index`. */
int zk_dev_merkle_node(const uint32_t *d_nodes, size_t index, uint8_t out[32], void *stream);

/* ---- row leaves of a shared proof ------------------------------------------------------------------------------
 * A shared proof (zk_batch_prove_shared) with row leaves commits the M = 2^log_batch trace polynomials as ONE tree over N leaves, leaf i
 * holding the row (f_0[i], .., f_{M-1}[i]): the header opens with that tree's 2^ce_f digests of depth ce_f = min(c, L - 1) in one commit
 * (cap 0: one root), the 3M alphas and the rest of the header are unchanged; per query three tuples -- the rows x, x + B, x + 2B, each
 * the M values in statement order, a u64 count and ONE path of L - ce_f digests -- then the cp tuple and the group tuples as ever.
 * SHA-256 and the field hash only (no prover makes BLAKE2s row leaves). */
/* From the next zk_batch_prove_shared on (zk_batch_prove does not look at it; off at creation).  ZK_ERR_STATE while a call runs on the
 * batch.  After a shared proof with row leaves tree 0 is the one tree over the rows, not the batch's f heap: it answers
 * zk_batch_merkle_nodes / zk_batch_merkle_cap with ZK_ERR_STATE until the next zk_batch_prove or shared proof without row leaves. */
int zk_batch_set_shared_rows(zk_batch *b, int on);
int zk_batch_get_shared_rows(const zk_batch *b);
/* zk_proof_data_len_shared with row leaves: zk_proof_data_len_cap of the other arguments plus 12 (M - 1) (1 + q) -- the further alphas
 * and 4 (M - 1) more value bytes in each of the 3 q row tuples.  row_leaves = 0: zk_proof_data_len_shared.  0 where that returns 0, or
 * for row_leaves with log_batch = 0. */
size_t zk_proof_data_len_shared_rows(uint32_t log_n, uint32_t log_blowup, uint32_t n_queries, uint32_t grind_bits, uint32_t fold_log,
                                     int coset_leaves, uint32_t stop_log, uint32_t cap_log, uint32_t log_batch, int row_leaves);
/* zk_verify_shared for proofs with row leaves; row_leaves = 0 runs the same lines and gives every input zk_verify_shared's answer.
 * With row leaves: -1 sizes, layout, any length other than zk_proof_data_len_shared_rows of the arguments; -2 the sum over the statements
 * at x (f_p(x) is value p of row x) against the cp value opened; -3 the three row path lengths and cp's; -4 / -5 / -6 the path of row
 * x / x + B / x + 2B against cap entry leaf >> (L - ce_f); all others as ever.  The strict replay commits the f cap in one piece and
 * counts 3M + G + q challenges.  row_leaves with log_batch outside 1..8 or with hash_kind 2 (BLAKE2s): *check_out = -1 and
 * ZK_ERR_INVALID. */
int zk_verify_shared_rows(const uint8_t *proof, size_t len, const uint8_t *state, uint32_t log_n, uint32_t log_blowup,
                          const uint32_t *public_last, uint32_t log_batch, int hash_kind, uint32_t n_queries, uint32_t grind_bits,
                          uint32_t fold_log, int coset_leaves, uint32_t stop_log, uint32_t cap_log, int row_leaves, int32_t *check_out);
/* The digest of a row leaf of m values (m a power of two, 1 .. 256), hash_kind 0 or 1.  SHA-256: the digest of the 4m-byte message, each
 * value 4 bytes big-endian, in statement order.  Field hash: m <= 8 the coset leaf, compress(v_0 .. v_{m-1}, 0, .., 0, m); m >= 16 the
 * chain c_0 = compress(v_0 .. v_7, 0, .., 0, m), c_k = compress(c_{k-1} || v_8k .. v_8k+7), k < m / 8, whose last link is the digest. */
int zk_row_leaf_hash(const uint32_t *values, uint32_t m, int hash_kind, uint8_t out[32]);
/* The tree of a shared proof with row leaves, stand-alone: d_vals: [2^log_batch][2^log_len] u32 on the device (1 <= log_batch <= 8,
 * 1 <= log_len, log_len + log_batch <= 30), d_nodes: (2^(log_len + 1) - 1) * 8 u32 state words in heap order; hash_kind 0 or 1. */
int zk_dev_merkle_build_rows(const uint32_t *d_vals, uint32_t log_len, uint32_t log_batch, uint32_t *d_nodes, void *stream, int hash_kind);

#ifdef __cplusplus
}
#endif
#endif
