/* sharded_stub_driver.c -- the threads of the sharded batches under ThreadSanitizer, without a GPU (linked with lc3_host.c, lc3_packet.c and tools/stub_shim.c:
 * csrc/Makefile, target stub).  One sharded encoder and one sharded decoder of 3 shards, 200 calls each from the main thread, then destroy; then a second
 * pair, the encoder driven from one application thread and the decoder from another at the same time.  Exit status 0 and no report: the hand-over between
 * the calling thread and the workers is ordered. */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../include/lc3plus_batch.h"

enum { S = 7, SHARDS = 3, T = 4, N = 480, CALLS = 200, STRIDE = 160 };
int lc3stub_log(void* out, int max);
void lc3stub_reset(void);

static int fail(const char* what, int code) { fprintf(stderr, "sharded_stub_driver: %s: %d\n", what, code); return 1; }

static int drive_encoder(lc3plus_sharded* e)
{
    int16_t* pcm = (int16_t*)calloc((size_t)S * T * N, sizeof(int16_t));
    uint8_t* out = (uint8_t*)calloc((size_t)S * T, STRIDE);
    int rates[S * T], nb[S * T], rc = 0;
    if (!pcm || !out) return fail("calloc", 0);
    for (int i = 0; i < S * T; i++) rates[i] = 32000 + 16000 * (i % 5);
    for (int i = 0; i < CALLS && !rc; i++) {
        const LC3_Error r = lc3plus_enc_sharded_encode(e, pcm, 16, NULL, i & 1 ? rates : NULL, T, out, STRIDE, nb);
        if (r) rc = fail("lc3plus_enc_sharded_encode", r);
        if (!rc && nb[S * T - 1] != (i & 1 ? rates[S * T - 1] / 800 : 80)) rc = fail("num_bytes", nb[S * T - 1]);
    }
    free(pcm); free(out);
    return rc;
}
static int drive_decoder(lc3plus_dec_sharded* d)
{
    uint8_t* frames = (uint8_t*)calloc((size_t)S * T, STRIDE);
    int16_t* pcm = (int16_t*)calloc((size_t)S * T * N, sizeof(int16_t));
    uint8_t bfi[S * T], status[S * T];
    int sizes[S * T], rc = 0;
    if (!pcm || !frames) return fail("calloc", 0);
    for (int i = 0; i < S * T; i++) { sizes[i] = 40 + 20 * (i % 5); bfi[i] = i % 7 == 3; }
    for (int i = 0; i < CALLS && !rc; i++) {
        const LC3_Error r = lc3plus_dec_sharded_decode(d, frames, STRIDE, i & 1 ? sizes : NULL, bfi, T, pcm, 16, status);
        if (r) rc = fail("lc3plus_dec_sharded_decode", r);
    }
    free(pcm); free(frames);
    return rc;
}
static int make_pair(lc3plus_sharded** e, lc3plus_dec_sharded** d)
{
    int rates[S], sizes[S], devices[SHARDS] = {0, 0, 0};
    for (int i = 0; i < S; i++) { rates[i] = 64000; sizes[i] = 80; }
    LC3_Error r = lc3plus_enc_sharded_create(e, S, 48000, 1, 10.0f, 0, rates, devices, SHARDS);
    if (r) return fail("lc3plus_enc_sharded_create", r);
    r = lc3plus_dec_sharded_create(d, S, 48000, 1, 10.0f, 0, sizes, devices, SHARDS);
    if (r) return fail("lc3plus_dec_sharded_create", r);
    return 0;
}
static void* enc_thread(void* p) { return (void*)(intptr_t)drive_encoder((lc3plus_sharded*)p); }
static void* dec_thread(void* p) { return (void*)(intptr_t)drive_decoder((lc3plus_dec_sharded*)p); }

int main(void)
{
    lc3plus_sharded* e = NULL; lc3plus_dec_sharded* d = NULL;
    lc3stub_reset();
    if (make_pair(&e, &d) || drive_encoder(e) || drive_decoder(d)) return 1;
    if (lc3plus_enc_sharded_destroy(e) || lc3plus_dec_sharded_destroy(d)) return fail("destroy", 0);
    int n = lc3stub_log(NULL, 0);
    if (n != 2 * CALLS * SHARDS) return fail("calls logged", n);
    /* the second pair: two application threads at once, each with a sharded batch of its own */
    if (make_pair(&e, &d)) return 1;
    pthread_t te, td; void *re = NULL, *rd = NULL;
    if (pthread_create(&te, NULL, enc_thread, e) || pthread_create(&td, NULL, dec_thread, d)) return fail("pthread_create", 0);
    pthread_join(te, &re); pthread_join(td, &rd);
    if (re || rd) return 1;
    if (lc3plus_enc_sharded_destroy(e) || lc3plus_dec_sharded_destroy(d)) return fail("destroy", 0);
    n = lc3stub_log(NULL, 0);
    if (n != 4 * CALLS * SHARDS) return fail("calls logged", n);
    printf("sharded_stub_driver: %d calls on %d shards, ok\n", n, SHARDS);
    return 0;
}
