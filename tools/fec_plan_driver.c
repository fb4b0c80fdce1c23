/* fec_plan_driver.c -- lc3plus_plan_fec_encode, lc3plus_plan_fec_recover and the refusals of the FEC calls in a program of its own, built with lc3_host.c, lc3_packet.c and
 * tools/stub_shim.c under AddressSanitizer + UndefinedBehaviorSanitizer (make -C audio_codec_amd/csrc fec_driver; tests/test_fec_cpu.py runs it as a child
 * process).  Every array is a heap block of exactly the size the header names - the wire buffer, the accumulators, the FEC buffer, the ring and the workspace too
 * - so a read or write one element too far ends the program.
 *
 *   fec_plan_driver encode SEED ROUTES FRAMES GROUP STRIDE
 *       a stamped list over ROUTES x FRAMES cells with holes, bad routes and unstamped entries, a state and an accumulator of random words, counts, groups (GROUP
 *       < 0: random, also outside [0, 16]) and flush flags, drawn from SEED by the generator below (tests/test_fec_cpu.py draws the same); every output printed as
 *       one line of numbers
 *   fec_plan_driver recover SEED STREAMS N GROUP WINDOW
 *       N datagrams and N / GROUP FEC items of random bytes, most with a plausible FEC header planted in them
 *   fec_plan_driver refuse
 *       the refusals in the header's order on a NULL batch, on a zero-filled block in place of a batch and on the host plans */
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
#define WANT(x, rc) do { const int got_ = (int)(x); if (got_ != (int)(rc)) { printf("line %d: %s gave %d, not %d\n", __LINE__, #x, got_, (int)(rc)); return 1; } } while (0)

static int encode(char** v)
{
    lcg_x = (uint32_t)atoi(v[0]);
    const int R = atoi(v[1]), T = atoi(v[2]), k = atoi(v[3]), stride = atoi(v[4]);
    enum { ROOM = 12, A = 64 };
    if (R < 1 || T < 1 || stride < 1) return 2;
    const size_t cells = (size_t)R * T, m_max = cells + 2;
    int32_t* route = block(4 * m_max); int32_t* frame = block(4 * m_max); int64_t* offset = block(8 * m_max); int32_t* size = block(4 * m_max); uint8_t* status = block(m_max);
    long long at = 0;
    size_t n = 0;
    for (int r = 0; r < R; r++)
        for (int t = 0; t < T; t++) {
            const uint32_t d = lcg();
            if (d % 7 == 0) continue;
            const int nb = 1 + (int)(d % 90);
            at += lcg() & 3;
            route[n] = d % 23 ? r : R; frame[n] = t; offset[n] = at; size[n] = ROOM + nb; status[n] = d % 19 == 0 ? 0 : 1;
            at += ROOM + nb;
            n++;
        }
    const size_t m = n + 2;                                          /* two entries behind n_packets */
    int32_t* route2 = block(4 * m); int32_t* frame2 = block(4 * m); int64_t* offset2 = block(8 * m); int32_t* size2 = block(4 * m); uint8_t* status2 = block(m);
    memcpy(route2, route, 4 * n); memcpy(frame2, frame, 4 * n); memcpy(offset2, offset, 8 * n); memcpy(size2, size, 4 * n); memcpy(status2, status, n);
    for (size_t p = n; p < m; p++) { route2[p] = 0; frame2[p] = 0; offset2[p] = 0; size2[p] = 0; status2[p] = 1; }
    uint8_t* wire = block((size_t)at);
    for (long long i = 0; i < at; i++) wire[i] = (uint8_t)lcg();
    int32_t* state_in = block(32 * (size_t)R); uint8_t* acc_in = block((size_t)R * A);
    for (int i = 0; i < R * A; i++) acc_in[i] = (uint8_t)lcg();
    for (int r = 0; r < R; r++) {
        const int K = 1 + (int)(lcg() % 16), F = (int)(lcg() % (uint32_t)(K + 1)), mx = (int)(lcg() % (A + 8)) - 4;
        int32_t* st = state_in + 8 * r;
        st[0] = F; st[1] = K; st[2] = (int32_t)(lcg() & 0xFFFF); st[3] = (int32_t)(lcg() & 0xFFFF); st[4] = (int32_t)(lcg() & 0xFFFF); st[5] = (int32_t)lcg();
        st[6] = (int32_t)(lcg() & 0xFFFF); st[7] = mx;
    }
    int32_t* stats = block(16 * (size_t)R);
    memset(stats, 0, 16 * (size_t)R);
    for (int r = 0; r < R; r++) stats[4 * r] = (int32_t)(lcg() % (uint32_t)(T + 2)) - 1;
    int32_t* group = block(4 * (size_t)R); uint8_t* flush = block((size_t)R); int32_t* seq_base = block(4 * (size_t)R); int32_t* fec_seq_base = block(4 * (size_t)R);
    for (int r = 0; r < R; r++) group[r] = k >= 0 ? k : (int32_t)(lcg() % 19) - 1;
    for (int r = 0; r < R; r++) { flush[r] = (uint8_t)(lcg() & 1); seq_base[r] = (65000 + 300 * r) & 0xFFFF; fec_seq_base[r] = 10 * r; }
    const long long Q = (long long)cells - 2 > 1 ? (long long)cells - 2 : 1;
    const long long cap = (long long)(lcg() % (uint32_t)(Q * stride + 1));
    uint8_t* fec_wire = block((size_t)cap);
    int32_t* state_out = block(32 * (size_t)R); uint8_t* acc_out = block((size_t)R * A);
    int64_t* n_packets = block(8); int64_t* n_fec = block(8);
    *n_packets = (int64_t)n;
    int32_t* f_route = block(4 * (size_t)Q); int32_t* f_seq = block(4 * (size_t)Q); int32_t* f_frame = block(4 * (size_t)Q); int64_t* f_off = block(8 * (size_t)Q);
    int32_t* f_size = block(4 * (size_t)Q); uint8_t* f_flags = block((size_t)Q); int32_t* f_mask = block(4 * (size_t)Q); int32_t* next = block(4 * (size_t)R);
    int32_t* rs_out = block(16 * (size_t)R);
    void* work = block((size_t)lc3plus_fec_work_bytes(R, T));
    const LC3_Error e = lc3plus_plan_fec_encode((int64_t)m, n_packets, route2, frame2, offset2, size2, status2, wire, at, ROOM, 0, R, T, seq_base, stats, group, flush,
                                                fec_seq_base, state_in, acc_in, state_out, acc_out, A, fec_wire, cap, stride, 12, Q, n_fec, f_route, f_seq, f_frame, f_off,
                                                f_size, f_flags, f_mask, next, rs_out, work, NULL, 0);
    printf("rc %d\n", (int)e);
    if (e) return 0;
    PRINT("n_fec", n_fec, 1, " %lld", long long); PRINT("fec_route", f_route, Q, " %d", int); PRINT("fec_seq", f_seq, Q, " %d", int); PRINT("fec_frame", f_frame, Q, " %d", int);
    PRINT("fec_offset", f_off, Q, " %lld", long long); PRINT("fec_size", f_size, Q, " %d", int); PRINT("fec_flags", f_flags, Q, " %d", int);
    PRINT("fec_mask", f_mask, Q, " %d", int); PRINT("next_fec_seq", next, R, " %d", int); PRINT("route_stats", rs_out, 4 * R, " %d", int);
    PRINT("state", state_out, 8 * R, " %d", int); PRINT("acc", acc_out, R * A, " %d", int); PRINT("fec_wire", fec_wire, cap, " %d", int);
    /* once more with next_fec_seq in place: the records keep their numbers, and fec_seq_base becomes what next_fec_seq was */
    {
        const long long nq = *n_fec < Q ? *n_fec : Q;
        int32_t* seq1 = block(4 * (size_t)Q);
        memcpy(seq1, f_seq, 4 * (size_t)Q);
        if (lc3plus_plan_fec_encode((int64_t)m, n_packets, route2, frame2, offset2, size2, status2, wire, at, ROOM, 0, R, T, seq_base, stats, group, flush, fec_seq_base,
                                    state_in, acc_in, state_out, acc_out, A, fec_wire, cap, stride, 12, Q, n_fec, f_route, f_seq, f_frame, f_off, f_size, f_flags, f_mask,
                                    fec_seq_base, rs_out, work, NULL, 0))
            return 1;
        if (memcmp(seq1, f_seq, 4 * (size_t)nq) || memcmp(fec_seq_base, next, 4 * (size_t)R)) { printf("next_fec_seq in place changed the numbers\n"); return 1; }
        for (int r = 0; r < R; r++) fec_seq_base[r] = 10 * r;
        free(seq1);
    }
    /* once more with every optional input and output NULL */
    if (lc3plus_plan_fec_encode((int64_t)m, n_packets, route2, frame2, offset2, size2, NULL, wire, at, ROOM, 0, R, T, seq_base, NULL, group, NULL, fec_seq_base, NULL, NULL,
                                NULL, NULL, 0, fec_wire, cap, stride, 12, Q, n_fec, f_route, f_seq, f_frame, f_off, f_size, NULL, NULL, NULL, NULL, work, NULL, 0))
        return 1;
    free(route); free(frame); free(offset); free(size); free(status); free(route2); free(frame2); free(offset2); free(size2); free(status2); free(wire); free(state_in);
    free(acc_in); free(stats); free(group); free(flush); free(seq_base); free(fec_seq_base); free(fec_wire); free(state_out); free(acc_out); free(n_packets); free(n_fec);
    free(f_route); free(f_seq); free(f_frame); free(f_off); free(f_size); free(f_flags); free(f_mask); free(next); free(rs_out); free(work);
    return 0;
}

static int recover(char** v)
{
    lcg_x = (uint32_t)atoi(v[0]);
    const int S = atoi(v[1]), n = atoi(v[2]), k = atoi(v[3]), window = atoi(v[4]);
    if (S < 1 || n < 1 || k < 1 || k > 16) return 2;
    const int nf = (n + k - 1) / k, rec_stride = 48;
    int64_t* off = block(8 * (size_t)n); int32_t* size = block(4 * (size_t)n); int32_t* stream = block(4 * (size_t)n); int32_t* seq = block(4 * (size_t)n);
    long long at = 0;
    for (int i = 0; i < n; i++) {
        at += lcg() & 3;
        off[i] = at; size[i] = 12 + (int32_t)(lcg() % 50); stream[i] = (int32_t)(lcg() % (uint32_t)(S + 2)) - 1;
        seq[i] = (i + (lcg() % 3 == 0)) & 0xFFFF;
        at += size[i];
    }
    int64_t* foff = block(8 * (size_t)nf); int32_t* fsize = block(4 * (size_t)nf); int32_t* fstream = block(4 * (size_t)nf);
    for (int f = 0; f < nf; f++) {
        at += lcg() & 3;
        foff[f] = at; fsize[f] = 10 + (int32_t)(lcg() % 70); fstream[f] = (int32_t)(lcg() % (uint32_t)(S + 1));
        at += fsize[f];
    }
    const long long rec_offset = at;
    const long long cap = at + (long long)nf * rec_stride - (long long)(lcg() % 20);
    uint8_t* ring = block((size_t)cap);
    for (long long i = 0; i < cap; i++) ring[i] = (uint8_t)lcg();
    for (int f = 0; f < nf; f++) {
        if (lcg() % 4 && fsize[f] >= 18) {
            uint8_t* a = ring + foff[f];
            a[0] &= (uint8_t)(0x3F | (lcg() % 5 == 0 ? 0x40 : 0));
            a[2] = (uint8_t)((f * k) >> 8); a[3] = (uint8_t)(f * k);
            a[10] = 0; a[11] = (uint8_t)(lcg() % 60);
            const unsigned mask = (0xFFFFu << (16 - k)) & 0xFFFFu;
            a[12] = (uint8_t)(mask >> 8); a[13] = (uint8_t)mask;
        }
    }
    if (n > 3) { off[0] = -1; size[1] = 5; foff[0] = at + 100000; }
    int32_t* ssrc = block(4 * (size_t)S);
    for (int s = 0; s < S; s++) ssrc[s] = 0x9000 + s;
    int64_t* r_off = block(8 * (size_t)nf); int32_t* r_size = block(4 * (size_t)nf); int32_t* r_seq = block(4 * (size_t)nf); uint8_t* st = block((size_t)nf);
    int32_t* stats = block(64);
    void* work = block((size_t)lc3plus_fec_recover_work_bytes(S, window));
    const LC3_Error e = lc3plus_plan_fec_recover(S, n, ring, cap, off, size, stream, seq, nf, fstream, foff, fsize, window, ssrc, rec_offset, rec_stride, r_off, r_size, r_seq,
                                                 st, stats, work, NULL, 0);
    printf("rc %d\n", (int)e);
    if (e) return 0;
    PRINT("ring", ring, cap, " %d", int); PRINT("rec_dg_offsets", r_off, nf, " %lld", long long); PRINT("rec_dg_sizes", r_size, nf, " %d", int);
    PRINT("rec_seq", r_seq, nf, " %d", int); PRINT("status", st, nf, " %d", int); PRINT("stats", stats, 16, " %d", int);
    if (lc3plus_plan_fec_recover(S, n, ring, cap, off, size, stream, seq, nf, fstream, foff, fsize, window, ssrc, rec_offset, rec_stride, r_off, r_size, r_seq, NULL, NULL,
                                 work, NULL, 0))
        return 1;
    free(off); free(size); free(stream); free(seq); free(foff); free(fsize); free(fstream); free(ring); free(ssrc); free(r_off); free(r_size); free(r_seq); free(st);
    free(stats); free(work);
    return 0;
}

/* an encode call's arguments; q[]: n_packets pkt_route pkt_frame pkt_offset pkt_size pkt_status wire seq_base route_stats group flush fec_seq_base state_in acc_in
 * state_out acc_out fec_wire n_fec fec_route fec_seq fec_frame fec_offset fec_size fec_flags fec_mask next_fec_seq route_stats_out work */
typedef struct { int64_t max_packets, wcap, fcap, fstride, max_fec; int room, proom, n_routes, n_frames, acc_stride, froom; void* q[28]; } eargs;
static const int e_required[] = {0, 1, 2, 3, 4, 6, 7, 9, 11, 16, 17, 18, 19, 20, 21, 22, 27};
static int ecall(int which, void* batch, const eargs* a)
{
    void* const* q = a->q;
#define EREST a->max_packets, q[0], q[1], q[2], q[3], q[4], q[5], q[6], a->wcap, a->room, a->proom, a->n_routes, a->n_frames, q[7], q[8], q[9], q[10], q[11], q[12], q[13], \
              q[14], q[15], a->acc_stride, q[16], a->fcap, a->fstride, a->froom, a->max_fec, q[17], q[18], q[19], q[20], q[21], q[22], q[23], q[24], q[25], q[26], q[27], NULL, 1
    if (which == 0) return lc3plus_enc_batch_fec_encode((lc3plus_batch*)batch, EREST);
    if (which == 1) return lc3plus_dec_batch_fec_encode((lc3plus_dec_batch*)batch, EREST);
    return lc3plus_plan_fec_encode(EREST);
}
/* a recover call's; q[]: ring dg_offsets dg_sizes stream seq fec_stream fec_offsets fec_num_bytes ssrc rec_dg_offsets rec_dg_sizes rec_seq status stats work */
typedef struct { int64_t n_items, cap, n_fec, rec_offset, rec_stride; int window; void* q[15]; } rargs;
static const int r_required[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14};
static int rcall(int which, void* batch, const rargs* a)
{
    void* const* q = a->q;
#define RREST a->n_items, q[0], a->cap, q[1], q[2], q[3], q[4], a->n_fec, q[5], q[6], q[7], a->window, q[8], a->rec_offset, a->rec_stride, q[9], q[10], q[11], q[12], q[13], \
              q[14], NULL, 1
    if (which == 0) return lc3plus_dec_batch_fec_recover((lc3plus_dec_batch*)batch, RREST);
    return lc3plus_plan_fec_recover(which - 1, RREST);               /* which - 1: n_streams */
}

static int refuse(void)
{
    void* tiny[28];
    for (int k = 0; k < 28; k++) { tiny[k] = block(512); memset(tiny[k], 0, 512); }
    void* fake = calloc(1, 4096);
    if (!fake) return 3;
    eargs eg = {1, 64, 64, 64, 1, 12, 0, 1, 1, 32, 12, {0}};
    memcpy(eg.q, tiny, sizeof eg.q);
    for (int which = 0; which < 3; which++) {                        /* both batch calls and the plan */
        void* b = which < 2 ? fake : NULL;
        if (which < 2) { eargs a = eg; a.n_frames = 0; a.q[0] = NULL; WANT(ecall(which, NULL, &a), LC3_NULL_ERROR); WANT(ecall(which, NULL, &eg), LC3_NULL_ERROR); }
        for (size_t k = 0; k < sizeof e_required / sizeof *e_required; k++) {
            eargs a = eg; a.q[e_required[k]] = NULL; WANT(ecall(which, b, &a), LC3_NULL_ERROR);
            a.n_frames = 0; a.fstride = 0; WANT(ecall(which, b, &a), LC3_NULL_ERROR);                     /* NULL first */
        }
#define EBAD(field, value) do { eargs a = eg; a.field = (value); WANT(ecall(which, b, &a), LC3_ERROR); } while (0)
        EBAD(max_packets, 0); EBAD(max_packets, -1); EBAD(max_packets, (1LL << 31) - 1); EBAD(wcap, -1); EBAD(proom, -1); EBAD(room, 11); EBAD(proom, 1); EBAD(n_routes, 0);
        EBAD(n_frames, 0); EBAD(q[12], NULL); EBAD(q[13], NULL); EBAD(q[14], NULL); EBAD(q[15], NULL); EBAD(acc_stride, 0); EBAD(acc_stride, 24); EBAD(q[14], tiny[12]);
        EBAD(q[15], tiny[13]); EBAD(q[14], (char*)tiny[12] + 16); EBAD(q[15], (char*)tiny[13] + 16); EBAD(fcap, -1); EBAD(fstride, 0); EBAD(fstride, (1LL << 30) + 1); EBAD(froom, 11); EBAD(froom, (1 << 20) + 1); EBAD(max_fec, 0);
        EBAD(q[16], tiny[6]);                                                                             /* the FEC buffer is the wire buffer */
        EBAD(q[27], (char*)tiny[27] + 4);                                                                 /* a work that is not 8-byte aligned */
        { eargs a = eg; a.n_routes = 1 << 16; a.n_frames = 1 << 15; WANT(ecall(which, b, &a), LC3_ERROR); }
    }
    WANT(ecall(2, NULL, &eg), LC3_OK);                                /* a good call: arrays of zeros */
    rargs rg = {1, 64, 1, 0, 32, 64, {0}};
    memcpy(rg.q, tiny, sizeof rg.q);
    for (int which = 0; which < 3; which += 2) {                     /* the batch call; the plan with n_streams 1 */
        void* b = which == 0 ? fake : NULL;
        if (which == 0) { rargs a = rg; a.n_items = 0; a.q[0] = NULL; WANT(rcall(0, NULL, &a), LC3_NULL_ERROR); WANT(rcall(0, NULL, &rg), LC3_NULL_ERROR); }
        for (size_t k = 0; k < sizeof r_required / sizeof *r_required; k++) {
            rargs a = rg; a.q[r_required[k]] = NULL; WANT(rcall(which, b, &a), LC3_NULL_ERROR);
            a.n_items = 0; a.window = 9; WANT(rcall(which, b, &a), LC3_NULL_ERROR);
        }
#define RBAD(field, value) do { rargs a = rg; a.field = (value); WANT(rcall(which, b, &a), LC3_ERROR); } while (0)
        RBAD(n_items, 0); RBAD(n_items, -1); RBAD(n_items, 1LL << 29); RBAD(cap, -1); RBAD(n_fec, 0); RBAD(n_fec, 1LL << 29); RBAD(window, 32); RBAD(window, 96);
        RBAD(window, 1 << 17); RBAD(rec_offset, -1); RBAD(rec_stride, 11); RBAD(rec_stride, (1LL << 30) + 1); RBAD(q[14], (char*)tiny[14] + 4);
    }
    WANT(rcall(1, NULL, &rg), LC3_ERROR);                             /* the plan with n_streams 0 */
    WANT(rcall(2, NULL, &rg), LC3_OK);
    for (size_t k = 0; k < 4096; k++) if (((unsigned char*)fake)[k]) { printf("the batch was written\n"); return 1; }
    for (int k = 0; k < 28; k++) free(tiny[k]);
    free(fake);
    printf("refusals ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 7 && !strcmp(argv[1], "encode")) return encode(argv + 2);
    if (argc == 7 && !strcmp(argv[1], "recover")) return recover(argv + 2);
    if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse();
    fprintf(stderr, "usage: %s encode SEED ROUTES FRAMES GROUP STRIDE | recover SEED STREAMS N GROUP WINDOW | refuse\n", argv[0]);
    return 2;
}
