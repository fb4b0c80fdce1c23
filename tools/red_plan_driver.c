/* red_plan_driver.c -- lc3plus_plan_red_pack, lc3plus_plan_red_unpack and the refusals of the RED calls in a program of its own, built with lc3_host.c, lc3_packet.c and
 * tools/stub_shim.c under AddressSanitizer + UndefinedBehaviorSanitizer (make -C audio_codec_amd/csrc red_driver; tests/test_red_cpu.py runs it as a child
 * process).  Every array is a heap block of exactly the size the header names - the frames, the tails, the ring and the wire buffer too - so a read or write one
 * element too far ends the program.
 *
 *   red_plan_driver pack SEED N DEPTH HEADER_ROOM ALIGN
 *       a list of N + 2 packets, N of them in front of n_packets, over 3 streams x 6 frames and 4 routes with tails, drawn from SEED by the generator below
 *       (tests/test_red_cpu.py draws the same), packed with max_depth DEPTH; every output printed as one line of numbers
 *   red_plan_driver unpack SEED N MAX_RED
 *       N payloads of random bytes, half of them with a run of block headers in front, over 3 streams
 *   red_plan_driver refuse
 *       the refusals in the header's order on a NULL batch, on a zero-filled block in place of a batch and on the host plans; every array is a block of 64 bytes */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/lc3.h"
#include "../include/lc3plus_batch.h"

static uint32_t lcg_x;
static uint32_t lcg(void) { lcg_x = (lcg_x * 1103515245u + 12345u) & 0x7FFFFFFFu; return lcg_x >> 8; }

static void* block(size_t n) { void* p = malloc(n ? n : 1); if (!p) exit(3); memset(p, 0x5A, n ? n : 1); return p; }
#define PRINT(name, a, n, fmt, cast) do { printf("%s", name); for (long long i_ = 0; i_ < (long long)(n); i_++) printf(fmt, (cast)(a)[i_]); printf("\n"); } while (0)

static int pack(char** v)
{
    lcg_x = (uint32_t)atoi(v[0]);
    const int N = atoi(v[1]), D = atoi(v[2]), room = atoi(v[3]), align = atoi(v[4]);
    enum { S = 3, T = 6, R = 4, M = 60, STRIDE = 64 };
    if (N < 1 || D < 0 || D > 4) return 2;
    int32_t* nb = block(4 * S * T); int64_t* off = block(8 * S * T); uint8_t* flags = block(S * T);
    long long at = 0;
    for (int k = 0; k < S * T; k++) {
        const uint32_t d = lcg();
        nb[k] = d % 11 == 0 ? 0 : d % 13 == 0 ? M + 5 : 1 + (int32_t)(d % M);
        flags[k] = (uint8_t)(d >> 4 & 3);
        at += lcg() & 3;
        off[k] = at;
        at += nb[k] <= M ? nb[k] : 0;
    }
    uint8_t* frames = block((size_t)at);
    for (long long k = 0; k < at; k++) frames[k] = (uint8_t)lcg();
    int32_t* counts = block(4 * S); int32_t* route_src = block(4 * R); int32_t* depth = block(4 * R); int32_t* pt = block(4 * R);
    for (int s = 0; s < S; s++) counts[s] = (int32_t)(lcg() % (T + 3)) - 1;
    for (int r = 0; r < R; r++) route_src[r] = (int32_t)(lcg() % (S + 1));
    for (int r = 0; r < R; r++) { depth[r] = (int32_t)(lcg() % 7) - 1; pt[r] = 96 + r; }
    const size_t m = (size_t)N + 2;
    int32_t* route = block(4 * m); int32_t* frame = block(4 * m);
    for (size_t p = 0; p < m; p++) route[p] = (int32_t)(lcg() % (R + 2)) - 1;
    for (size_t p = 0; p < m; p++) frame[p] = (int32_t)(lcg() % (T + 2)) - 1;
    int32_t* tz_in = block(4 * (size_t)S * D); uint8_t* tb_in = block((size_t)S * D * STRIDE);
    for (int k = 0; k < S * D; k++) tz_in[k] = (int32_t)(lcg() % (STRIDE + 8)) - 4;
    for (int k = 0; k < S * D * STRIDE; k++) tb_in[k] = (uint8_t)lcg();
    const long long cap = (long long)(lcg() % (uint32_t)(N * (room + 80) + 1));
    uint8_t* wire = block((size_t)cap);
    int32_t* tz_out = block(4 * (size_t)S * D); uint8_t* tb_out = block((size_t)S * D * STRIDE);
    int64_t* n_packets = block(8);
    *n_packets = N;
    int64_t* r_off = block(8 * m); int32_t* r_size = block(4 * m); uint8_t* r_flags = block(m); uint8_t* r_blocks = block(m); int64_t* total = block(8);
    int32_t* stats = block(16 * R);
    void* work = block((size_t)lc3plus_red_work_bytes((int64_t)m));
    const LC3_Error e = lc3plus_plan_red_pack(S, T, frames, at, off, nb, M, flags, 2, counts, R, route_src, (int64_t)m, n_packets, route, frame, D, depth, pt, 480,
                                              room + 150, tb_in, tz_in, STRIDE, tb_out, tz_out, wire, cap, room, align, r_off, r_size, r_flags, r_blocks, total, stats,
                                              work, NULL, 0);
    printf("rc %d\n", (int)e);
    if (e) return 0;
    PRINT("red_offset", r_off, m, " %lld", long long); PRINT("red_size", r_size, m, " %d", int); PRINT("red_flags", r_flags, m, " %d", int);
    PRINT("red_blocks", r_blocks, m, " %d", int); PRINT("wire_total", total, 1, " %lld", long long); PRINT("route_stats", stats, 4 * R, " %d", int);
    PRINT("tail_sizes", tz_out, S * D, " %d", int); PRINT("tail_bytes", tb_out, S * D * STRIDE, " %d", int); PRINT("wire", wire, cap, " %d", int);
    /* once more with every optional input and output NULL */
    if (lc3plus_plan_red_pack(S, T, frames, at, off, nb, M, NULL, 0, NULL, S, NULL, (int64_t)m, n_packets, route, frame, D, NULL, pt, 480, room + 150, NULL, NULL, STRIDE,
                              NULL, NULL, wire, cap, room, align, r_off, r_size, NULL, NULL, NULL, NULL, work, NULL, 0))
        return 1;
    free(nb); free(off); free(flags); free(frames); free(counts); free(route_src); free(depth); free(pt); free(route); free(frame); free(tz_in); free(tb_in); free(wire);
    free(tz_out); free(tb_out); free(n_packets); free(r_off); free(r_size); free(r_flags); free(r_blocks); free(total); free(stats); free(work);
    return 0;
}

static void header(uint8_t* b, int pt, int to, int len)
{
    const uint32_t w = 1u << 31 | (uint32_t)(pt & 127) << 24 | (uint32_t)(to & 0x3FFF) << 10 | (uint32_t)(len & 0x3FF);
    b[0] = (uint8_t)(w >> 24); b[1] = (uint8_t)(w >> 16); b[2] = (uint8_t)(w >> 8); b[3] = (uint8_t)w;
}

static int unpack(char** v)
{
    lcg_x = (uint32_t)atoi(v[0]);
    const int N = atoi(v[1]), max_red = atoi(v[2]), S = 3;
    if (N < 1 || max_red < 0 || max_red > 4) return 2;
    int64_t* off = block(8 * (size_t)N); int32_t* size = block(4 * (size_t)N);
    long long at = 0;
    for (int i = 0; i < N; i++) { at += lcg() & 3; off[i] = at; size[i] = (int32_t)(lcg() % 41); at += size[i]; }
    uint8_t* ring = block((size_t)at);
    for (long long k = 0; k < at; k++) ring[k] = (uint8_t)lcg();
    for (int i = 0; i < N; i++)
        if (lcg() & 1) {                                             /* a run of block headers and a final byte, so that the later checks are reached */
            const int k = (int)(lcg() % 6);
            long long p = off[i];
            for (int j = 0; j < k; j++)
                if (p + 4 <= off[i] + size[i]) {
                    const int pt = 96 + (int)(lcg() & 1), to = 480 * (int)(lcg() % 4), odd = lcg() % 5 == 0, len = (int)(lcg() % 9);
                    header(ring + p, pt, to + odd, len);
                    p += 4;
                }
            if (p < off[i] + size[i]) ring[p] = (uint8_t)(96 + (lcg() % 3 == 0));
        }
    int32_t* stream = block(4 * (size_t)N); int32_t* seq = block(4 * (size_t)N); int32_t* ts = block(4 * (size_t)N); int32_t* pt = block(4 * (size_t)S);
    for (int i = 0; i < N; i++) { stream[i] = (int32_t)(lcg() % 5) - 1; seq[i] = (i * 3) & 0xFFFF; ts[i] = (int32_t)(0xFFFFFE00u + 480u * (uint32_t)i); }
    pt[0] = 96; pt[1] = -1; pt[2] = 97;
    if (N > 3) { off[0] = -1; size[1] = -5; off[2] = at; size[2] = 1; }     /* out of range: never read */
    const size_t m = (size_t)N * ((size_t)max_red + 1);
    int32_t* o_stream = block(4 * m); int32_t* o_seq = block(4 * m); int64_t* o_off = block(8 * m); int32_t* o_nb = block(4 * m); int32_t* o_ts = block(4 * m);
    uint8_t* o_gen = block(m); uint8_t* o_st = block((size_t)N); int32_t* stats = block(4 * LC3PLUS_RED_UNPACK_STATS_WORDS);
    const LC3_Error e = lc3plus_plan_red_unpack(S, N, stream, seq, off, size, ts, ring, at, max_red, pt, 480, o_stream, o_seq, o_off, o_nb, o_ts, o_gen, o_st, stats, NULL, 0);
    printf("rc %d\n", (int)e);
    if (e) return 0;
    PRINT("stream", o_stream, m, " %d", int); PRINT("seq", o_seq, m, " %d", int); PRINT("offsets", o_off, m, " %lld", long long); PRINT("num_bytes", o_nb, m, " %d", int);
    PRINT("timestamp", o_ts, m, " %d", int); PRINT("gen", o_gen, m, " %d", int); PRINT("status", o_st, N, " %d", int);
    PRINT("stats", stats, LC3PLUS_RED_UNPACK_STATS_WORDS, " %d", int);
    /* once more with every optional input and output NULL */
    if (lc3plus_plan_red_unpack(S, N, stream, seq, off, size, NULL, ring, at, max_red, NULL, 480, o_stream, o_seq, o_off, o_nb, NULL, NULL, NULL, NULL, NULL, 0)) return 1;
    free(off); free(size); free(ring); free(stream); free(seq); free(ts); free(pt); free(o_stream); free(o_seq); free(o_off); free(o_nb); free(o_ts); free(o_gen); free(o_st);
    free(stats);
    return 0;
}

#define WANT(x, code) do { const int got_ = (x); if (got_ != (code)) { printf("line %d: %d, not %d\n", __LINE__, got_, (int)(code)); return 1; } } while (0)

/* a pack call's arguments; q[]: frames offsets num_bytes flags counts route_src n_packets pkt_route pkt_frame depth block_pt tail_bytes_in tail_sizes_in tail_bytes_out
 * tail_sizes_out wire red_offset red_size red_flags red_blocks wire_total route_stats work */
typedef struct { int n_frames, mfb, n_routes, depth, ts_step, mpb, stride, room, align; int64_t fcap, wcap, max_packets; void* q[23]; } kargs;
static const int k_required[] = {0, 1, 2, 6, 7, 8, 10, 15, 16, 17, 22};
static int kcall(int which, void* batch, const kargs* a)
{
    void* const* q = a->q;
#define KREST a->n_frames, q[0], a->fcap, q[1], q[2], a->mfb, q[3], 0, q[4], a->n_routes, q[5], a->max_packets, q[6], q[7], q[8], a->depth, q[9], q[10], a->ts_step, a->mpb, \
              q[11], q[12], a->stride, q[13], q[14], q[15], a->wcap, a->room, a->align, q[16], q[17], q[18], q[19], q[20], q[21], q[22], NULL, 1
    if (which == 0) return lc3plus_enc_batch_red_pack((lc3plus_batch*)batch, KREST);
    if (which == 1) return lc3plus_dec_batch_red_pack((lc3plus_dec_batch*)batch, KREST);
    return lc3plus_plan_red_pack(which - 2, KREST);                  /* which - 2: n_streams */
}
/* an unpack call's; q[]: stream seq offsets num_bytes timestamp ring block_pt out_stream out_seq out_offsets out_num_bytes out_timestamp out_gen status stats */
typedef struct { int64_t n_items, cap; int max_red, ts_step; void* q[15]; } uargs;
static const int u_required[] = {0, 1, 2, 3, 5, 7, 8, 9, 10};
static int ucall(int which, void* batch, const uargs* a)
{
    void* const* q = a->q;
#define UREST a->n_items, q[0], q[1], q[2], q[3], q[4], q[5], a->cap, a->max_red, q[6], a->ts_step, q[7], q[8], q[9], q[10], q[11], q[12], q[13], q[14], NULL, 1
    if (which == 0) return lc3plus_dec_batch_red_unpack((lc3plus_dec_batch*)batch, UREST);
    return lc3plus_plan_red_unpack(which - 1, UREST);                /* which - 1: n_streams */
}

static int refuse(void)
{
    void* tiny[23];
    for (int k = 0; k < 23; k++) { tiny[k] = block(64); memset(tiny[k], 0, 64); }
    void* fake = calloc(1, 4096);
    if (!fake) return 3;
    kargs kg = {1, 40, 1, 1, 480, 1400, 48, 12, 1, 100, 100, 1, {0}};
    memcpy(kg.q, tiny, sizeof kg.q);
    for (int which = 0; which < 4; which++) {                        /* both batch calls; the plan with n_streams 1 */
        if (which == 2) continue;
        void* b = which < 2 ? fake : NULL;
        if (which < 2) { kargs a = kg; a.n_frames = 0; a.q[0] = NULL; WANT(kcall(which, NULL, &a), LC3_NULL_ERROR); WANT(kcall(which, NULL, &kg), LC3_NULL_ERROR); }
        for (size_t k = 0; k < sizeof k_required / sizeof *k_required; k++) {
            kargs a = kg; a.q[k_required[k]] = NULL; WANT(kcall(which, b, &a), LC3_NULL_ERROR);
            a.n_frames = 0; a.depth = 9; WANT(kcall(which, b, &a), LC3_NULL_ERROR);                       /* NULL first */
        }
#define KBAD(field, value) do { kargs a = kg; a.field = (value); WANT(kcall(which, b, &a), LC3_ERROR); } while (0)
        KBAD(n_frames, 0); KBAD(n_frames, -1); KBAD(n_routes, 0); KBAD(mfb, 0); KBAD(fcap, -1); KBAD(wcap, -1); KBAD(max_packets, 0); KBAD(max_packets, -1);
        KBAD(max_packets, 1LL << 31); KBAD(depth, -1); KBAD(depth, 5); KBAD(ts_step, 0); KBAD(ts_step, -1); KBAD(mpb, -1); KBAD(stride, 40); KBAD(stride, 32);
        KBAD(room, -1); KBAD(room, INT32_MAX); KBAD(align, 0); KBAD(align, 3); KBAD(align, 8192);
        KBAD(q[11], NULL); KBAD(q[12], NULL); KBAD(q[13], NULL); KBAD(q[14], NULL);                       /* one of a tail's two arrays without the other */
        KBAD(q[22], (char*)tiny[22] + 4);                                                                 /* a work that is not 8-byte aligned */
        { kargs a = kg; a.n_routes = 2; a.q[5] = NULL; WANT(kcall(which, b, &a), LC3_ERROR); }            /* no route_src and n_routes != n_streams */
    }
    WANT(kcall(2, NULL, &kg), LC3_ERROR);                             /* the plan with n_streams 0 */
    WANT(kcall(3, NULL, &kg), LC3_OK);                                /* and a good call: a list of no packets */
    uargs ug = {1, 64, 1, 480, {0}};
    memcpy(ug.q, tiny, sizeof ug.q);
    for (int which = 0; which < 3; which += 2) {                     /* the batch call; the plan with n_streams 1 */
        void* b = which == 0 ? fake : NULL;
        if (which == 0) { uargs a = ug; a.n_items = 0; a.q[0] = NULL; WANT(ucall(0, NULL, &a), LC3_NULL_ERROR); WANT(ucall(0, NULL, &ug), LC3_NULL_ERROR); }
        for (size_t k = 0; k < sizeof u_required / sizeof *u_required; k++) {
            uargs a = ug; a.q[u_required[k]] = NULL; WANT(ucall(which, b, &a), LC3_NULL_ERROR);
            a.n_items = 0; a.max_red = 9; WANT(ucall(which, b, &a), LC3_NULL_ERROR);
        }
#define UBAD(field, value) do { uargs a = ug; a.field = (value); WANT(ucall(which, b, &a), LC3_ERROR); } while (0)
        UBAD(n_items, 0); UBAD(n_items, -1); UBAD(n_items, 1LL << 29); UBAD(cap, -1); UBAD(max_red, -1); UBAD(max_red, 5); UBAD(ts_step, 0); UBAD(ts_step, -7);
    }
    WANT(ucall(1, NULL, &ug), LC3_ERROR);                             /* the plan with n_streams 0 */
    for (size_t k = 0; k < 4096; k++) if (((unsigned char*)fake)[k]) { printf("the batch was written\n"); return 1; }
    for (int k = 0; k < 23; k++) free(tiny[k]);
    free(fake);
    printf("refusals ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 7 && !strcmp(argv[1], "pack")) return pack(argv + 2);
    if (argc == 5 && !strcmp(argv[1], "unpack")) return unpack(argv + 2);
    if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse();
    fprintf(stderr, "usage: %s pack SEED N DEPTH HEADER_ROOM ALIGN | unpack SEED N MAX_RED | refuse\n", argv[0]);
    return 2;
}
