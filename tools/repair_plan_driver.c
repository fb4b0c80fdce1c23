/* repair_plan_driver.c -- lc3plus_plan_fec_repair and the refusals of the repair call in a program of its own, built with lc3_host.c, lc3_packet.c and
 * tools/stub_shim.c under AddressSanitizer + UndefinedBehaviorSanitizer (make -C audio_codec_amd/csrc repair_driver; tests/test_fec_repair_cpu.py runs it as a
 * child process).  Every array is a heap block of exactly the size the header names - the ring, the stores, each call's item arrays and outputs, the workspace -
 * so a read or write one element too far ends the program.
 *
 *   repair_plan_driver run FILE
 *       a receiver's session, read from FILE as numbers: S H P med_stride fec_stride passes area calls, the S SSRCs, then per call n_items n_fec, the media
 *       items (offset size stream seq each) on one line, the FEC items on the next, and the `area` bytes of the ring in front of the history.  The stores start
 *       zeroed and are carried from call to call; the workspace is filled with 0xA5 before every call.  Every call's outputs are printed as lines of numbers
 *       behind their names, a blank line between calls, the stores after the last call at the end
 *   repair_plan_driver refuse
 *       the refusals in the header's order on a NULL batch and on the host plan */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/lc3.h"
#include "../include/lc3plus_batch.h"

static void* block(size_t n, int fill) { void* p = malloc(n ? n : 1); if (!p) exit(3); memset(p, fill, n ? n : 1); return p; }
static long long num(FILE* f) { long long v; if (fscanf(f, "%lld", &v) != 1) exit(4); return v; }
#define PRINT(name, a, n, fmt, cast) do { printf("%s:", name); for (long long i_ = 0; i_ < (long long)(n); i_++) printf(fmt, (cast)(a)[i_]); printf("\n"); } while (0)
#define WANT(x, rc) do { const int got_ = (int)(x); if (got_ != (int)(rc)) { printf("line %d: %s gave %d, not %d\n", __LINE__, #x, got_, (int)(rc)); return 1; } } while (0)

static int run(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    const int S = (int)num(f), H = (int)num(f), P = (int)num(f), ms = (int)num(f), fs = (int)num(f), passes = (int)num(f);
    const long long area = num(f);
    const int calls = (int)num(f);
    if (S < 1 || H < 1 || P < 1 || ms < 1 || fs < 1 || area < 0 || (area & 15)) return 2;
    const size_t nh = (size_t)S * H, np = (size_t)S * P, cap = (size_t)area + nh * ms;
    int32_t* ssrc = block(4 * (size_t)S, 0);
    for (int s = 0; s < S; s++) ssrc[s] = (int32_t)(uint32_t)num(f);
    uint8_t* ring = block(cap, 0);
    int32_t* med_seq = block(4 * nh, 0); int32_t* med_size = block(4 * nh, 0); uint8_t* store = block(np * fs, 0);
    int32_t* cell_seq = block(4 * np, 0); int32_t* cell_size = block(4 * np, 0); uint8_t* cell_status = block(np, 0); int32_t* state = block(16 * (size_t)S, 0);
    const int64_t wb = lc3plus_fec_repair_work_bytes(S, H, P);
    if (wb <= 0) return 2;
    for (int c = 0; c < calls; c++) {
        const long long n = num(f), m = num(f);
        int64_t* off = block(8 * (size_t)n, 0x5A); int32_t* size = block(4 * (size_t)n, 0x5A); int32_t* stream = block(4 * (size_t)n, 0x5A); int32_t* seq = block(4 * (size_t)n, 0x5A);
        int64_t* foff = block(8 * (size_t)m, 0x5A); int32_t* fsize = block(4 * (size_t)m, 0x5A); int32_t* fstream = block(4 * (size_t)m, 0x5A); int32_t* fseq = block(4 * (size_t)m, 0x5A);
        for (long long i = 0; i < n; i++) { off[i] = num(f); size[i] = (int32_t)num(f); stream[i] = (int32_t)num(f); seq[i] = (int32_t)num(f); }
        for (long long i = 0; i < m; i++) { foff[i] = num(f); fsize[i] = (int32_t)num(f); fstream[i] = (int32_t)num(f); fseq[i] = (int32_t)num(f); }
        for (long long i = 0; i < area; i++) ring[i] = (uint8_t)num(f);
        int64_t* rec_off = block(8 * np, 0x5A); int32_t* rec_size = block(4 * np, 0x5A); int32_t* rec_seq = block(4 * np, 0x5A);
        uint8_t* item_status = block((size_t)n, 0x5A); uint8_t* fec_status = block((size_t)m, 0x5A); int32_t* stats = block(4 * LC3PLUS_FEC_STATS_WORDS, 0x5A);
        void* work = block((size_t)wb, 0xA5);
        const int rc = lc3plus_plan_fec_repair(S, n, ring, (int64_t)cap, n ? off : NULL, n ? size : NULL, n ? stream : NULL, n ? seq : NULL, m, m ? fstream : NULL,
                                               m ? foff : NULL, m ? fsize : NULL, m ? fseq : NULL, ssrc, area, H, ms, med_seq, med_size, store, P, fs, cell_seq, cell_size,
                                               cell_status, state, passes, rec_off, rec_size, rec_seq, item_status, fec_status, stats, work, NULL, 0);
        printf("rc: %d\n", rc);
        PRINT("rec_dg_offsets", rec_off, np, " %lld", long long); PRINT("rec_dg_sizes", rec_size, np, " %d", int); PRINT("rec_seq", rec_seq, np, " %d", int);
        PRINT("item_status", item_status, n, " %d", int); PRINT("fec_status", fec_status, m, " %d", int); PRINT("stats", stats, LC3PLUS_FEC_STATS_WORDS, " %d", int);
        printf("\n");
        free(off); free(size); free(stream); free(seq); free(foff); free(fsize); free(fstream); free(fseq);
        free(rec_off); free(rec_size); free(rec_seq); free(item_status); free(fec_status); free(stats); free(work);
    }
    fclose(f);
    PRINT("ring", ring + area, cap - (size_t)area, " %d", int); PRINT("med_seq", med_seq, nh, " %d", int); PRINT("med_size", med_size, nh, " %d", int);
    PRINT("fec_store", store, np * fs, " %d", int); PRINT("cell_seq", cell_seq, np, " %d", int); PRINT("cell_size", cell_size, np, " %d", int);
    PRINT("cell_status", cell_status, np, " %d", int); PRINT("state", state, 4 * (size_t)S, " %d", int);
    free(ssrc); free(ring); free(med_seq); free(med_size); free(store); free(cell_seq); free(cell_size); free(cell_status); free(state);
    return 0;
}

/* the arguments of a good call; every refusal below changes one of them */
typedef struct {
    int S; int64_t n; uint8_t* ring; int64_t cap; int64_t* off; int32_t* size; int32_t* stream; int32_t* seq; int64_t m; int32_t* fstream; int64_t* foff; int32_t* fsize;
    int32_t* fseq; int32_t* ssrc; int64_t mo; int H; int ms; int32_t* med_seq; int32_t* med_size; uint8_t* store; int P; int fs; int32_t* cell_seq; int32_t* cell_size;
    uint8_t* cell_status; int32_t* state; int passes; int64_t* rec_off; int32_t* rec_size; int32_t* rec_seq; uint8_t* is; uint8_t* fst; int32_t* stats; void* work;
} args;
static int plan(const args* a)
{
    return lc3plus_plan_fec_repair(a->S, a->n, a->ring, a->cap, a->off, a->size, a->stream, a->seq, a->m, a->fstream, a->foff, a->fsize, a->fseq, a->ssrc, a->mo, a->H, a->ms,
                                   a->med_seq, a->med_size, a->store, a->P, a->fs, a->cell_seq, a->cell_size, a->cell_status, a->state, a->passes, a->rec_off, a->rec_size,
                                   a->rec_seq, a->is, a->fst, a->stats, a->work, NULL, 0);
}
static int batch(lc3plus_dec_batch* b, const args* a)
{
    return lc3plus_dec_batch_fec_repair(b, a->n, a->ring, a->cap, a->off, a->size, a->stream, a->seq, a->m, a->fstream, a->foff, a->fsize, a->fseq, a->ssrc, a->mo, a->H, a->ms,
                                        a->med_seq, a->med_size, a->store, a->P, a->fs, a->cell_seq, a->cell_size, a->cell_status, a->state, a->passes, a->rec_off,
                                        a->rec_size, a->rec_seq, a->is, a->fst, a->stats, a->work, NULL, 0);
}
#define WITH(field, value, rc) do { args b_ = good; b_.field = (value); WANT(plan(&b_), rc); } while (0)

static int refuse(void)
{
    enum { S = 2, H = 16, P = 4, MS = 64, FS = 64, AREA = 256 };
    const size_t nh = S * H, np = S * P;
    args good = {S, 1, block(AREA + nh * MS, 0), AREA + nh * MS, block(8, 0), block(4, 0), block(4, 0), block(4, 0), 1, block(4, 0), block(8, 0), block(4, 0), block(4, 0),
                 block(4 * S, 0), AREA, H, MS, block(4 * nh, 0), block(4 * nh, 0), block(np * FS, 0), P, FS, block(4 * np, 0), block(4 * np, 0), block(np, 0), block(16 * S, 0),
                 1, block(8 * np, 0), block(4 * np, 0), block(4 * np, 0), block(1, 0), block(1, 0), block(4 * LC3PLUS_FEC_STATS_WORDS, 0),
                 block((size_t)lc3plus_fec_repair_work_bytes(S, H, P), 0xA5)};
    good.size[0] = 20; good.fsize[0] = 20; good.foff[0] = 32;
    WANT(plan(&good), LC3_OK);
    WANT(batch(NULL, &good), LC3_NULL_ERROR);
    /* the NULLs, each also beside a range error: the NULL is found first */
    WITH(ring, NULL, LC3_NULL_ERROR); WITH(ssrc, NULL, LC3_NULL_ERROR); WITH(med_seq, NULL, LC3_NULL_ERROR); WITH(med_size, NULL, LC3_NULL_ERROR);
    WITH(store, NULL, LC3_NULL_ERROR); WITH(cell_seq, NULL, LC3_NULL_ERROR); WITH(cell_size, NULL, LC3_NULL_ERROR); WITH(cell_status, NULL, LC3_NULL_ERROR);
    WITH(state, NULL, LC3_NULL_ERROR); WITH(rec_off, NULL, LC3_NULL_ERROR); WITH(rec_size, NULL, LC3_NULL_ERROR); WITH(rec_seq, NULL, LC3_NULL_ERROR);
    WITH(work, NULL, LC3_NULL_ERROR); WITH(off, NULL, LC3_NULL_ERROR); WITH(size, NULL, LC3_NULL_ERROR); WITH(stream, NULL, LC3_NULL_ERROR); WITH(seq, NULL, LC3_NULL_ERROR);
    WITH(fstream, NULL, LC3_NULL_ERROR); WITH(foff, NULL, LC3_NULL_ERROR); WITH(fsize, NULL, LC3_NULL_ERROR); WITH(fseq, NULL, LC3_NULL_ERROR);
    { args b = good; b.passes = 0; b.ring = NULL; WANT(plan(&b), LC3_NULL_ERROR); }
    WITH(is, NULL, LC3_OK); WITH(fst, NULL, LC3_OK); WITH(stats, NULL, LC3_OK);
    { args b = good; b.n = 0; b.off = NULL; b.size = NULL; b.stream = NULL; b.seq = NULL; WANT(plan(&b), LC3_OK); }
    { args b = good; b.m = 0; b.fstream = NULL; b.foff = NULL; b.fsize = NULL; b.fseq = NULL; WANT(plan(&b), LC3_OK); }
    /* the ranges */
    WITH(S, 0, LC3_ERROR); WITH(n, -1, LC3_ERROR); WITH(n, 1LL << 29, LC3_ERROR); WITH(m, -1, LC3_ERROR); WITH(m, 1LL << 29, LC3_ERROR); WITH(cap, -1, LC3_ERROR);
    WITH(mo, -16, LC3_ERROR); WITH(mo, AREA + 8, LC3_ERROR); WITH(H, 8, LC3_ERROR); WITH(H, 24, LC3_ERROR); WITH(H, 2048, LC3_ERROR);
    WITH(ms, 0, LC3_ERROR); WITH(ms, 72, LC3_ERROR); WITH(ms, (1 << 20) + 16, LC3_ERROR);
    WITH(P, 2, LC3_ERROR); WITH(P, 6, LC3_ERROR); WITH(P, 512, LC3_ERROR); WITH(fs, 0, LC3_ERROR); WITH(fs, 40, LC3_ERROR); WITH(fs, (1 << 20) + 16, LC3_ERROR);
    WITH(passes, 0, LC3_ERROR); WITH(passes, 5, LC3_ERROR);
    /* n_streams * H, then n_streams * P, of 2^31, under a ring_capacity that such a history would fit: no other check refuses these */
    { args b = good; b.S = 1 << 21; b.H = 1024; b.ms = 16; b.cap = 1LL << 40; WANT(plan(&b), LC3_ERROR); }
    { args b = good; b.S = 1 << 23; b.P = 256; b.ms = 16; b.cap = 1LL << 40; WANT(plan(&b), LC3_ERROR); }
    WITH(cap, good.cap - 1, LC3_ERROR); WITH(mo, AREA + 16, LC3_ERROR);          /* a history that ends behind the ring */
    /* overlaps */
    WITH(store, good.ring + AREA + 64, LC3_ERROR); WITH(med_size, good.med_seq, LC3_ERROR); WITH(cell_size, good.cell_seq + 1, LC3_ERROR);
    WITH(state, (int32_t*)good.cell_seq, LC3_ERROR); WITH(cell_status, (uint8_t*)good.med_size + 5, LC3_ERROR);
    WITH(work, (char*)good.work + 4, LC3_ERROR);
    WANT(lc3plus_fec_repair_work_bytes(0, H, P), 0); WANT(lc3plus_fec_repair_work_bytes(S, 8, P), 0); WANT(lc3plus_fec_repair_work_bytes(S, H, 3), 0);
    void* const all[] = {good.ring, good.off, good.size, good.stream, good.seq, good.fstream, good.foff, good.fsize, good.fseq, good.ssrc, good.med_seq, good.med_size,
                         good.store, good.cell_seq, good.cell_size, good.cell_status, good.state, good.rec_off, good.rec_size, good.rec_seq, good.is, good.fst, good.stats,
                         good.work};
    for (size_t i = 0; i < sizeof all / sizeof all[0]; i++) free(all[i]);
    printf("refusals ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "run")) return run(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse();
    fprintf(stderr, "usage: repair_plan_driver run FILE | refuse\n");
    return 2;
}
