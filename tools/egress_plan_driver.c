/* egress_plan_driver.c -- lc3plus_plan_egress and the refusals of the egress calls in a program of its own, built with lc3_host.c, lc3_packet.c and tools/stub_shim.c under
 * AddressSanitizer + UndefinedBehaviorSanitizer (make -C audio_codec_amd/csrc egress_driver; tests/test_egress_cpu.py runs it as a child process).  Every array
 * is a heap block of exactly the size the header names, so a read or write one element too far ends the program.
 *
 *   egress_plan_driver plan SEED S T R ORDER BITS HEADER_ROOM ALIGN WIRE_CAP   (WIRE_CAP < 0: in place)
 *       a case drawn from SEED by the generator below (tests/test_egress_cpu.py draws the same one), planned; every output printed as one line of numbers
 *   egress_plan_driver refuse
 *       the refusals in the header's order on a NULL batch, on a zero-filled block in place of a batch and on the host plan; the arrays of a call refused
 *       for its shape are blocks of 8 bytes, n_routes * n_frames at its limit and one below it */
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

static int plan(char** v)
{
    lcg_x = (uint32_t)atoi(v[0]);
    const int S = atoi(v[1]), T = atoi(v[2]), R = atoi(v[3]), order = atoi(v[4]), bits = atoi(v[5]), room = atoi(v[6]), align = atoi(v[7]);
    const long long wcap = atoll(v[8]);
    const size_t cells = (size_t)S * T, n = (size_t)R * T;
    int64_t* offsets = block(8 * cells); int32_t* nb = block(4 * cells); uint8_t* flags = block(cells);
    int32_t* counts = block(4 * (size_t)S); int32_t* src = block(4 * (size_t)R); int32_t* base = block(4 * (size_t)R);
    long long at = 0;
    for (size_t k = 0; k < cells; k++) {
        const uint32_t d = lcg();
        at += d & 3;
        nb[k] = d % 7 == 0 ? 0 : d % 11 == 0 ? -3 : d % 13 == 0 ? 41 : 1 + (int32_t)(d >> 4) % 40;
        offsets[k] = d % 17 == 0 ? -1 : at;
        if (nb[k] > 0 && nb[k] <= 40) at += nb[k];
        flags[k] = (uint8_t)(lcg() & 15);
    }
    const long long cap = at > 5 ? at - 5 : at;                      /* the last frames end beyond the capacity */
    uint8_t* frames = block((size_t)cap);
    for (long long k = 0; k < cap; k++) frames[k] = (uint8_t)lcg();
    for (int s = 0; s < S; s++) counts[s] = (int32_t)(lcg() % (uint32_t)(T + 3)) - 1;
    for (int r = 0; r < R; r++) { src[r] = (int32_t)(lcg() % (uint32_t)(S + 2)) - 1; base[r] = 65530 + r % 6; }
    int32_t* p_route = block(4 * n); int32_t* p_seq = block(4 * n); int32_t* p_frame = block(4 * n); int64_t* p_off = block(8 * n); int32_t* p_size = block(4 * n);
    uint8_t* p_flags = block(n); int64_t* n_packets = block(8); int64_t* total = block(8); int32_t* next_seq = block(4 * (size_t)R);
    int32_t* stats = block(16 * (size_t)R); uint8_t* status = block(n);
    uint8_t* wire = wcap >= 0 ? block((size_t)wcap) : NULL;
    void* work = block((size_t)lc3plus_egress_work_bytes(R, T));
    const LC3_Error e = lc3plus_plan_egress(S, T, frames, cap, offsets, nb, 40, flags, 8, counts, R, src, base, bits, order, wire, wcap >= 0 ? wcap : 0, room, align,
                                            p_route, p_seq, p_frame, p_off, p_size, p_flags, n_packets, total, next_seq, stats, status, work, NULL, 0);
    printf("rc %d\n", (int)e);
    if (e) return 0;
    printf("n_packets %lld\nwire_total %lld\n", (long long)*n_packets, (long long)*total);
    PRINT("pkt_route", p_route, *n_packets, " %d", int); PRINT("pkt_seq", p_seq, *n_packets, " %d", int); PRINT("pkt_frame", p_frame, *n_packets, " %d", int);
    PRINT("pkt_offset", p_off, *n_packets, " %lld", long long); PRINT("pkt_size", p_size, *n_packets, " %d", int); PRINT("pkt_flags", p_flags, *n_packets, " %d", int);
    PRINT("next_seq", next_seq, R, " %d", int); PRINT("stats", stats, 4 * R, " %d", int); PRINT("cell_status", status, n, " %d", int);
    PRINT("wire", wire, wcap >= 0 ? wcap : 0, " %d", int);
    for (size_t k = (size_t)*n_packets; k < n; k++)                  /* the list's tail is not written */
        if (p_route[k] != 0x5A5A5A5A || p_seq[k] != 0x5A5A5A5A || p_frame[k] != 0x5A5A5A5A || p_size[k] != 0x5A5A5A5A || p_flags[k] != 0x5A ||
            p_off[k] != 0x5A5A5A5A5A5A5A5ALL) { printf("tail written at %zu\n", k); return 1; }
    free(offsets); free(nb); free(flags); free(counts); free(src); free(base); free(frames); free(p_route); free(p_seq); free(p_frame); free(p_off); free(p_size);
    free(p_flags); free(n_packets); free(total); free(next_seq); free(stats); free(status); free(wire); free(work);
    return 0;
}

/* one call's arguments; q[] are the pointers in the header's order: frames offsets num_bytes flags counts route_src seq_base wire pkt_route pkt_seq pkt_frame
 * pkt_offset pkt_size pkt_flags n_packets wire_total next_seq stats cell_status work */
typedef struct { int n_frames, max_bytes, n_routes, bits, order, room, align; int64_t fcap, wcap; void* q[20]; } args;
enum { Q_FRAMES, Q_OFFSETS, Q_NB, Q_FLAGS, Q_COUNTS, Q_SRC, Q_BASE, Q_WIRE, Q_ROUTE, Q_SEQ, Q_FRAME, Q_OFF, Q_SIZE, Q_PFLAGS, Q_NP, Q_TOTAL, Q_NEXT, Q_STATS, Q_STATUS, Q_WORK };
static const int required[] = {Q_FRAMES, Q_OFFSETS, Q_NB, Q_BASE, Q_ROUTE, Q_SEQ, Q_FRAME, Q_OFF, Q_SIZE, Q_NP, Q_WORK};
#define REST(a) (a).n_frames, (a).q[0], (a).fcap, (a).q[1], (a).q[2], (a).max_bytes, (a).q[3], 0, (a).q[4], (a).n_routes, (a).q[5], (a).q[6], (a).bits, (a).order, (a).q[7], (a).wcap, \
                (a).room, (a).align, (a).q[8], (a).q[9], (a).q[10], (a).q[11], (a).q[12], (a).q[13], (a).q[14], (a).q[15], (a).q[16], (a).q[17], (a).q[18], (a).q[19], NULL, 1
static int call(int which, void* batch, const args* a)
{
    if (which == 0) return lc3plus_enc_batch_egress((lc3plus_batch*)batch, REST(*a));
    if (which == 1) return lc3plus_dec_batch_egress((lc3plus_dec_batch*)batch, REST(*a));
    return lc3plus_plan_egress(which - 2, REST(*a));                 /* which - 2: n_streams */
}
#define WANT(x, code) do { const int got_ = (x); if (got_ != (code)) { printf("line %d: %d, not %d\n", __LINE__, got_, (int)(code)); return 1; } } while (0)

static int refuse(void)
{
    void* tiny[20];
    for (int k = 0; k < 20; k++) tiny[k] = block(8);
    void* fake = calloc(1, 4096);
    if (!fake) return 3;
    args good = {1, 10, 1, 16, 0, 0, 1, 100, 100, {0}};
    memcpy(good.q, tiny, sizeof tiny);
    for (int which = 0; which < 4; which++) {                        /* the encoder's call, the decoder's, the plan with n_streams 1 */
        if (which == 2) continue;
        void* b = which < 2 ? fake : NULL;
        if (which < 2) { args a = good; a.n_frames = 0; a.q[Q_FRAMES] = NULL; WANT(call(which, NULL, &a), LC3_NULL_ERROR); WANT(call(which, NULL, &good), LC3_NULL_ERROR); }
        for (size_t k = 0; k < sizeof required / sizeof *required; k++) {
            args a = good; a.q[required[k]] = NULL; WANT(call(which, b, &a), LC3_NULL_ERROR);
            a.n_frames = 0; a.bits = 3; a.align = 3; WANT(call(which, b, &a), LC3_NULL_ERROR);           /* NULL first */
        }
#define BAD(field, value) do { args a = good; a.field = (value); WANT(call(which, b, &a), LC3_ERROR); } while (0)
        BAD(n_frames, 0); BAD(n_frames, -1); BAD(n_routes, 0); BAD(n_routes, -7); BAD(max_bytes, 0); BAD(max_bytes, -1); BAD(fcap, -1); BAD(wcap, -1);
        BAD(order, 2); BAD(order, -1); BAD(bits, 0); BAD(bits, 15); BAD(bits, 24); BAD(bits, 64); BAD(room, -1); BAD(room, INT32_MAX); BAD(align, 0); BAD(align, 3);
        BAD(align, 8192); BAD(align, -4);
        { args a = good; a.n_routes = 65536; a.n_frames = 32768; WANT(call(which, b, &a), LC3_ERROR); }     /* 2^31 cells: refused, the 8-byte arrays untouched */
        { args a = good; a.n_routes = INT32_MAX; a.q[Q_SRC] = NULL; WANT(call(which < 2 ? which : 7, b, &a), LC3_ERROR); }   /* one below: the route check answers */
        { args a = good; a.q[Q_WIRE] = NULL; a.room = 4; WANT(call(which, b, &a), LC3_ERROR); a.room = 0; a.align = 2; WANT(call(which, b, &a), LC3_ERROR); }
        { args a = good; a.q[Q_SRC] = NULL; a.n_routes = 3; WANT(call(which < 2 ? which : 4, b, &a), LC3_ERROR); }        /* identity routes: n_routes != n_streams */
        { args a = good; a.q[Q_WORK] = (char*)tiny[Q_WORK] + 4; WANT(call(which, b, &a), LC3_ERROR); }
    }
    { args a = good; WANT(call(2, NULL, &a), LC3_ERROR); WANT(call(1, NULL, &a), LC3_NULL_ERROR); }       /* the plan with n_streams 0 */
    if (lc3plus_egress_work_bytes(0, 4) || lc3plus_egress_work_bytes(4, 0) || lc3plus_egress_work_bytes(65536, 32768) || lc3plus_egress_work_bytes(3, 5) <= 0) return 1;
    for (size_t k = 0; k < 4096; k++) if (((unsigned char*)fake)[k]) { printf("the batch was written\n"); return 1; }
    for (int k = 0; k < 20; k++) {
        for (int j = 0; j < 8; j++) if (((unsigned char*)tiny[k])[j] != 0x5A) { printf("array %d was written\n", k); return 1; }
        free(tiny[k]);
    }
    free(fake);
    printf("refusals ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 11 && !strcmp(argv[1], "plan")) return plan(argv + 2);
    if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse();
    fprintf(stderr, "usage: %s plan SEED S T R ORDER BITS HEADER_ROOM ALIGN WIRE_CAP | refuse\n", argv[0]);
    return 2;
}
