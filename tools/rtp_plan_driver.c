/* rtp_plan_driver.c -- lc3plus_plan_rtp_parse, lc3plus_plan_rtp_stamp, lc3plus_rtp_sort_ssrc and the refusals of the RTP calls in a program of its own, built
 * with lc3_host.c, lc3_packet.c and tools/stub_shim.c under AddressSanitizer + UndefinedBehaviorSanitizer (make -C audio_codec_amd/csrc rtp_driver; tests/test_rtp_cpu.py runs
 * it as a child process).  Every array is a heap block of exactly the size the header names - the ring and the wire buffer too - so a read or write one element
 * too far ends the program.
 *
 *   rtp_plan_driver parse SEED N K ROOM
 *       N datagrams over a table of K senders (K <= 16) and 3 streams, drawn from SEED by the generator below (tests/test_rtp_cpu.py draws the same), parsed with
 *       payload_room ROOM; every output printed as one line of numbers
 *   rtp_plan_driver stamp SEED N HEADER_ROOM PAYLOAD_ROOM MODE
 *       a list of N + 2 packets, N of them in front of n_packets, over 3 routes x 4 frames, stamped with marker mode MODE
 *   rtp_plan_driver refuse
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

static int parse(char** v)
{
    lcg_x = (uint32_t)atoi(v[0]);
    const int N = atoi(v[1]), K = atoi(v[2]), room = atoi(v[3]), S = 3;
    if (N < 1 || K < 1 || K > 16) return 2;
    int32_t* key = block(4 * (size_t)K); int32_t* strm = block(4 * (size_t)K); int32_t* pt = block(4 * (size_t)S);
    for (int k = 0; k < K; k++) { key[k] = (int32_t)((uint32_t)k * 0x0F0F0F0Fu + 5u); strm[k] = k % 5 - 1; }
    pt[0] = 96; pt[1] = -1; pt[2] = 97;
    int64_t* off = block(8 * (size_t)N); int32_t* size = block(4 * (size_t)N);
    long long at = 0;
    for (int i = 0; i < N; i++) { at += lcg() & 3; off[i] = at; size[i] = (int32_t)(lcg() % 61); at += size[i]; }
    uint8_t* ring = block((size_t)at);
    for (long long k = 0; k < at; k++) ring[k] = (uint8_t)lcg();
    for (int i = 0; i < N; i++)
        if ((lcg() & 1) && size[i] >= 12) {                           /* an RTP header of version 2 from a known sender, so that the later checks are reached */
            uint8_t* b = ring + off[i];
            const uint32_t k = (uint32_t)key[lcg() % (uint32_t)K];
            b[0] = (uint8_t)(0x80 | (b[0] & 0x33));
            b[1] = (uint8_t)((b[1] & 0x80) | ((lcg() & 1) ? 96 : 97));
            b[8] = (uint8_t)(k >> 24); b[9] = (uint8_t)(k >> 16); b[10] = (uint8_t)(k >> 8); b[11] = (uint8_t)k;
            if (b[0] & 0x20) b[size[i] - 1] = (uint8_t)(lcg() % 4);
        }
    if (N > 3) { off[0] = -1; size[1] = -5; off[2] = at; size[2] = 1; }     /* out of range: never read */
    int32_t* o_stream = block(4 * (size_t)N); int32_t* o_seq = block(4 * (size_t)N); int64_t* o_off = block(8 * (size_t)N); int32_t* o_nb = block(4 * (size_t)N);
    int32_t* o_ts = block(4 * (size_t)N); uint8_t* o_m = block((size_t)N); uint8_t* o_st = block((size_t)N); int32_t* stats = block(4 * LC3PLUS_RTP_STATS_WORDS);
    const LC3_Error e = lc3plus_plan_rtp_parse(S, N, ring, at, off, size, K, key, strm, pt, room, o_stream, o_seq, o_off, o_nb, o_ts, o_m, o_st, stats, NULL, 0);
    printf("rc %d\n", (int)e);
    if (e) return 0;
    PRINT("stream", o_stream, N, " %d", int); PRINT("seq", o_seq, N, " %d", int); PRINT("offsets", o_off, N, " %lld", long long); PRINT("num_bytes", o_nb, N, " %d", int);
    PRINT("timestamp", o_ts, N, " %d", int); PRINT("marker", o_m, N, " %d", int); PRINT("status", o_st, N, " %d", int);
    PRINT("stats", stats, LC3PLUS_RTP_STATS_WORDS, " %d", int);
    /* once more with every optional output NULL */
    if (lc3plus_plan_rtp_parse(S, N, ring, at, off, size, K, key, strm, NULL, room, o_stream, o_seq, o_off, o_nb, NULL, NULL, NULL, NULL, NULL, 0)) return 1;
    free(key); free(strm); free(pt); free(off); free(size); free(ring); free(o_stream); free(o_seq); free(o_off); free(o_nb); free(o_ts); free(o_m); free(o_st);
    free(stats);
    return 0;
}

static int stamp(char** v)
{
    lcg_x = (uint32_t)atoi(v[0]);
    const int N = atoi(v[1]), room = atoi(v[2]), proom = atoi(v[3]), mode = atoi(v[4]), R = 3, T = 4;
    if (N < 1 || room < 12) return 2;
    const size_t m = (size_t)N + 2;
    int32_t* route = block(4 * m); int32_t* seq = block(4 * m); int32_t* frame = block(4 * m); int64_t* off = block(8 * m); int32_t* size = block(4 * m);
    uint8_t* flags = block(m);
    long long at = 0;
    for (size_t p = 0; p < m; p++) {
        const uint32_t d = lcg();
        route[p] = d % 9 == 0 ? -1 : d % 11 == 0 ? R : (int32_t)(d % (uint32_t)R);
        frame[p] = d % 13 == 0 ? T : (int32_t)((d >> 3) % (uint32_t)T);
        size[p] = d % 17 == 0 ? room - 1 : room + 1 + (int32_t)((d >> 5) % 20);
        flags[p] = (uint8_t)(d % 7 == 0);
        seq[p] = 65533 + (int32_t)p;
        off[p] = d % 19 == 0 ? -1 : at;
        at += size[p] + (lcg() & 3);
    }
    const long long wcap = at > 3 ? at - 3 : at;                     /* the last packet may end beyond the capacity */
    uint8_t* wire = block((size_t)wcap);
    uint8_t* cs = block((size_t)R * T); uint8_t* resume = block((size_t)R); int32_t* rs = block(16 * (size_t)R);
    for (int k = 0; k < R * T; k++) cs[k] = (uint8_t)(lcg() & 1);
    for (int r = 0; r < R; r++) { resume[r] = (uint8_t)(lcg() & 1); rs[4 * r] = (int32_t)(lcg() % (uint32_t)(T + 3)) - 1; rs[4 * r + 1] = rs[4 * r + 2] = rs[4 * r + 3] = 0; }
    int32_t* ssrc = block(4 * (size_t)R); int32_t* base = block(4 * (size_t)R); int32_t* pt = block(4 * (size_t)R);
    for (int r = 0; r < R; r++) { ssrc[r] = (int32_t)(0x80000001u + (uint32_t)r * 0x3FFFFFFFu); base[r] = (int32_t)(0xFFFFFF00u + (uint32_t)r * 100u); pt[r] = 96 + r; }
    int64_t* n_packets = block(8);
    *n_packets = N;
    uint8_t* status = block(m); int32_t* next_ts = block(4 * (size_t)R); uint8_t* next_resume = block((size_t)R);
    const LC3_Error e = lc3plus_plan_rtp_stamp((int64_t)m, n_packets, route, seq, frame, off, size, flags, R, T, ssrc, base, pt, 480, mode, cs, resume, rs, wire, wcap, room,
                                               proom, status, next_ts, next_resume, NULL, 0);
    printf("rc %d\n", (int)e);
    if (e) return 0;
    PRINT("pkt_status", status, m, " %d", int); PRINT("next_ts", next_ts, R, " %d", int); PRINT("next_resume", next_resume, R, " %d", int);
    PRINT("wire", wire, wcap, " %d", int);
    /* once more with every optional input and output NULL */
    if (lc3plus_plan_rtp_stamp((int64_t)m, n_packets, route, seq, frame, off, size, NULL, R, T, ssrc, base, pt, 480, 0, NULL, NULL, NULL, wire, wcap, room, proom, NULL, NULL,
                               NULL, NULL, 0))
        return 1;
    free(route); free(seq); free(frame); free(off); free(size); free(flags); free(wire); free(cs); free(resume); free(rs); free(ssrc); free(base); free(pt);
    free(n_packets); free(status); free(next_ts); free(next_resume);
    return 0;
}

#define WANT(x, code) do { const int got_ = (x); if (got_ != (code)) { printf("line %d: %d, not %d\n", __LINE__, got_, (int)(code)); return 1; } } while (0)

/* a parse call's arguments; q[]: ring dg_offsets dg_sizes ssrc_key ssrc_stream payload_type stream seq offsets num_bytes timestamp marker status stats */
typedef struct { int64_t n_items, cap; int n_ssrc, room; void* q[14]; } pargs;
static const int p_required[] = {0, 1, 2, 3, 4, 6, 7, 8, 9};
static int pcall(int which, void* batch, const pargs* a)
{
    void* const* q = a->q;
    if (which == 0)
        return lc3plus_dec_batch_rtp_parse((lc3plus_dec_batch*)batch, a->n_items, q[0], a->cap, q[1], q[2], a->n_ssrc, q[3], q[4], q[5], a->room, q[6], q[7], q[8], q[9],
                                           q[10], q[11], q[12], q[13], NULL, 1);
    return lc3plus_plan_rtp_parse(which - 1, a->n_items, q[0], a->cap, q[1], q[2], a->n_ssrc, q[3], q[4], q[5], a->room, q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13],
                                  NULL, 1);                          /* which - 1: n_streams */
}
/* a stamp call's; q[]: n_packets route seq frame offset size flags ssrc ts_base payload_type cell_status resume route_stats wire pkt_status next_ts next_resume */
typedef struct { int64_t max_packets, wcap; int n_routes, n_frames, mode, room, proom; void* q[17]; } sargs;
static const int s_required[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 13};
static int scall(int which, void* batch, const sargs* a)
{
    void* const* q = a->q;
#define SREST a->max_packets, q[0], q[1], q[2], q[3], q[4], q[5], q[6], a->n_routes, a->n_frames, q[7], q[8], q[9], 480, a->mode, q[10], q[11], q[12], q[13], a->wcap, a->room, \
              a->proom, q[14], q[15], q[16], NULL, 1
    if (which == 0) return lc3plus_enc_batch_rtp_stamp((lc3plus_batch*)batch, SREST);
    if (which == 1) return lc3plus_dec_batch_rtp_stamp((lc3plus_dec_batch*)batch, SREST);
    return lc3plus_plan_rtp_stamp(SREST);
}

static int refuse(void)
{
    void* tiny[17];
    for (int k = 0; k < 17; k++) tiny[k] = block(64);
    void* fake = calloc(1, 4096);
    if (!fake) return 3;
    pargs pg = {1, 100, 1, 0, {0}};
    memcpy(pg.q, tiny, sizeof pg.q);
    for (int which = 0; which < 3; which += 2) {                     /* the batch call; the plan with n_streams 1 */
        void* b = which == 0 ? fake : NULL;
        if (which == 0) { pargs a = pg; a.n_items = 0; a.q[0] = NULL; WANT(pcall(0, NULL, &a), LC3_NULL_ERROR); WANT(pcall(0, NULL, &pg), LC3_NULL_ERROR); }
        for (size_t k = 0; k < sizeof p_required / sizeof *p_required; k++) {
            pargs a = pg; a.q[p_required[k]] = NULL; WANT(pcall(which, b, &a), LC3_NULL_ERROR);
            a.n_items = 0; a.room = -1; WANT(pcall(which, b, &a), LC3_NULL_ERROR);                    /* NULL first */
        }
#define PBAD(field, value) do { pargs a = pg; a.field = (value); WANT(pcall(which, b, &a), LC3_ERROR); } while (0)
        PBAD(n_items, 0); PBAD(n_items, -1); PBAD(n_items, 1LL << 29); PBAD(n_items, INT64_MAX); PBAD(cap, -1); PBAD(n_ssrc, 0); PBAD(n_ssrc, -3); PBAD(room, -1);
        PBAD(room, 4097);
    }
    WANT(pcall(1, NULL, &pg), LC3_ERROR);                             /* the plan with n_streams 0 */
    WANT(pcall(2, NULL, &pg), LC3_OK);                                /* and a good call: an offset far outside the ring, RANGE */
    if (*(int32_t*)tiny[6] != -1 || *(uint8_t*)tiny[12] != LC3PLUS_RTP_RANGE || ((int32_t*)tiny[13])[LC3PLUS_RTP_RANGE] != 1) { printf("the good parse call\n"); return 1; }
    for (int k = 0; k < 17; k++) memset(tiny[k], 0x5A, 64);
    sargs sg = {1, 100, 1, 1, 0, 12, 0, {0}};
    memcpy(sg.q, tiny, sizeof sg.q);
    for (int which = 0; which < 3; which++) {
        void* b = which < 2 ? fake : NULL;
        if (which < 2) { sargs a = sg; a.n_frames = 0; a.q[0] = NULL; WANT(scall(which, NULL, &a), LC3_NULL_ERROR); WANT(scall(which, NULL, &sg), LC3_NULL_ERROR); }
        for (size_t k = 0; k < sizeof s_required / sizeof *s_required; k++) {
            sargs a = sg; a.q[s_required[k]] = NULL; WANT(scall(which, b, &a), LC3_NULL_ERROR);
            a.n_frames = 0; a.mode = 7; WANT(scall(which, b, &a), LC3_NULL_ERROR);
        }
#define SBAD(field, value) do { sargs a = sg; a.field = (value); WANT(scall(which, b, &a), LC3_ERROR); } while (0)
        SBAD(max_packets, 0); SBAD(max_packets, -1); SBAD(n_routes, 0); SBAD(n_routes, -1); SBAD(n_frames, 0); SBAD(n_frames, -2); SBAD(wcap, -1); SBAD(proom, -1);
        SBAD(room, 11); SBAD(room, 0); SBAD(room, -1); SBAD(proom, 1); SBAD(proom, INT32_MAX); SBAD(mode, 2); SBAD(mode, -1);
        { sargs a = sg; a.mode = 1; a.q[10] = NULL; WANT(scall(which, b, &a), LC3_ERROR); }               /* AFTER_HOLE without cell_status */
        { sargs a = sg; a.q[10] = NULL; WANT(scall(which, b, &a), LC3_ERROR); a.q[16] = NULL; if (which == 2) WANT(scall(which, b, &a), LC3_OK); }   /* next_resume without it */
    }
    if (lc3plus_rtp_sort_ssrc(1, NULL, tiny[0]) != LC3_NULL_ERROR || lc3plus_rtp_sort_ssrc(1, tiny[0], NULL) != LC3_NULL_ERROR || lc3plus_rtp_sort_ssrc(0, tiny[0], tiny[1]) != LC3_ERROR)
        return 1;
    for (size_t k = 0; k < 4096; k++) if (((unsigned char*)fake)[k]) { printf("the batch was written\n"); return 1; }
    for (int k = 0; k < 14; k++)                                      /* the good stamp call of the plan wrote pkt_status[0] and next_ts[0], nothing else */
        for (int j = 0; j < 64; j++) if (((unsigned char*)tiny[k])[j] != 0x5A) { printf("array %d was written\n", k); return 1; }
    int32_t key[5] = {7, -1, 3, (int32_t)0x80000000u, 5}, val[5] = {0, 1, 2, 3, 4};
    if (lc3plus_rtp_sort_ssrc(5, key, val) != LC3_OK || key[0] != 3 || key[1] != 5 || key[2] != 7 || key[3] != (int32_t)0x80000000u || key[4] != -1 || val[0] != 2 ||
        val[1] != 4 || val[2] != 0 || val[3] != 3 || val[4] != 1)
        return 1;
    key[2] = 5;
    if (lc3plus_rtp_sort_ssrc(5, key, val) != LC3_ERROR) return 1;
    for (int k = 0; k < 17; k++) free(tiny[k]);
    free(fake);
    printf("refusals ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 6 && !strcmp(argv[1], "parse")) return parse(argv + 2);
    if (argc == 7 && !strcmp(argv[1], "stamp")) return stamp(argv + 2);
    if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse();
    fprintf(stderr, "usage: %s parse SEED N K ROOM | stamp SEED N HEADER_ROOM PAYLOAD_ROOM MODE | refuse\n", argv[0]);
    return 2;
}
