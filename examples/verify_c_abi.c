/* verify_c_abi.c -- check many proofs at once on the GPU, from plain C.
 *
 * Proves 64 proofs of the reference's size with zk_batch_*, corrupts one byte of one proof (a node of its f(x) path), and
 * verifies all 64 with one zk_verifier_run: strict (the transcript replay, as zk_verify_strict) and plain (the reference's
 * checks, proof.rs:15).  Prints the rejected index and the check it stopped at, which is the CPU verifier's number.
 *   gcc -O2 -Iinclude examples/verify_c_abi.c -Lzkstark_amd -lzkstark_amd -Wl,-rpath,$PWD/zkstark_amd -o verify_c_abi
 *   ./verify_c_abi [bad_index [fold_log]]
 * fold_log 2 or 3: the batch is proved with that FRI folding factor (zk_batch_set_fold) and the verifier follows it
 * (zk_verifier_set_fold); the CPU number then comes from zk_verify_fold.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "zkstark_amd.h"

static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

#define CHECK(call)                                                        \
    do {                                                                   \
        int rc_ = (call);                                                  \
        if (rc_ != ZK_OK) {                                                \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, zk_last_error()); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

/* prints every rejected proof; returns how many there were */
static size_t report(const char *mode, const int32_t *checks, size_t count) {
    size_t bad = 0;
    for (size_t p = 0; p < count; ++p)
        if (checks[p]) {
            printf("%s: proof %zu rejected at check %d\n", mode, p, checks[p]);
            ++bad;
        }
    printf("%s: %zu of %zu proofs accepted\n", mode, count - bad, count);
    return bad;
}

int main(int argc, char **argv) {
    const uint32_t log_n = 10, log_b = 3, log_batch = 6;               /* prover.rs:48-57, 64 proofs */
    size_t bad_index = argc > 1 ? (size_t)atoi(argv[1]) : 17;
    const uint32_t fold_log = argc > 2 ? (uint32_t)atoi(argv[2]) : 1;
    if (zk_abi_version() != ZK_ABI_VERSION) {                           /* the library on the path was built from another zkstark_amd.h */
        fprintf(stderr, "libzkstark_amd speaks ABI version %u, this program was compiled against %u\n", zk_abi_version(), ZK_ABI_VERSION);
        return 2;
    }
    zk_batch *b = NULL;
    CHECK(zk_batch_create(0, log_n, log_b, log_batch, &b));
    if (fold_log != 1) CHECK(zk_batch_set_fold(b, fold_log));
    size_t batch = zk_batch_size(b), plen = zk_proof_data_len_fold(log_n, log_b, 1, 0, fold_log);
    if (bad_index >= batch) bad_index = batch - 1;
    uint32_t *a0 = malloc(batch * 4), *a1 = malloc(batch * 4), *last = malloc(batch * 4);
    for (size_t p = 0; p < batch; ++p) { a0[p] = 1; a1[p] = 3141592 + (uint32_t)p; }
    CHECK(zk_batch_gen_fibsq(b, a0, a1));
    CHECK(zk_batch_public_last(b, last));
    uint8_t *proofs = malloc(batch * plen), *states = malloc(batch * 32);
    int32_t *checks = malloc(batch * sizeof(int32_t));
    CHECK(zk_batch_prove(b, proofs, plen, states));
    zk_batch_destroy(b);

    /* one byte of the first sibling of the f(x) path: after the roots and challenges (76 + 36 bytes per committed FRI layer: log_n
     * of them, or one per group of fold_log rounds), the free term (4), the query raw (4), f(x) (4) and the path's count (8) */
    const size_t layers = (log_n + fold_log - 1) / fold_log;
    proofs[bad_index * plen + 76 + 36 * layers + 4 + 4 + 4 + 8] ^= 0x01;

    zk_verifier *v = NULL;
    CHECK(zk_verifier_create(0, log_n, log_b, &v));
    if (fold_log != 1) CHECK(zk_verifier_set_fold(v, fold_log));
    int rc = zk_verifier_run(v, proofs, plen, batch, states, last, checks);      /* warm-up */
    double t0 = now_ms();
    rc = zk_verifier_run(v, proofs, plen, batch, states, last, checks);
    double ms = now_ms() - t0;
    if (rc != ZK_OK && rc != ZK_ERR_VERIFY) { fprintf(stderr, "zk_verifier_run -> %d: %s\n", rc, zk_last_error()); return 1; }
    if (rc == ZK_ERR_VERIFY) printf("zk_verifier_run: %s\n", zk_last_error());
    size_t bad = report("strict", checks, batch);
    printf("strict: %zu proofs in %.3f ms\n", batch, ms);
    rc = zk_verifier_run(v, proofs, plen, batch, NULL, last, checks);
    if (rc != ZK_OK && rc != ZK_ERR_VERIFY) { fprintf(stderr, "zk_verifier_run -> %d: %s\n", rc, zk_last_error()); return 1; }
    bad += report("plain", checks, batch);
    /* the CPU verifier's number for the same proof */
    int32_t cpu = 0;
    if (fold_log != 1) zk_verify_fold(proofs + bad_index * plen, plen, NULL, log_n, log_b, last[bad_index], ZK_HASH_SHA256, 1, 0, fold_log, &cpu);
    else zk_verify_check(proofs + bad_index * plen, plen, NULL, log_n, log_b, last[bad_index], ZK_HASH_SHA256, 1, &cpu);
    printf("cpu plain: proof %zu check %d\n", bad_index, cpu);
    zk_verifier_destroy(v);
    free(a0); free(a1); free(last); free(proofs); free(states); free(checks);
    return bad == 2 ? 0 : 1;
}
