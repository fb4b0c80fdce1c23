/* rtcp_plan_driver.c -- lc3plus_plan_rtcp_stats, lc3plus_rtcp_workspace_bytes and the refusals of lc3plus_dec_batch_rtcp_stats in a program of its own, built
 * with lc3_host.c, lc3_packet.c and tools/stub_shim.c under AddressSanitizer + UndefinedBehaviorSanitizer (make -C audio_codec_amd/csrc rtcp_driver; tests/test_rtcp_cpu.py
 * runs it as a child process).  Every array is a heap block of exactly the size the header names, so a read or write one element too far ends the program.
 *
 *   rtcp_plan_driver stats SEED N S REPORT INPLACE
 *       N items over S streams drawn from SEED by the generator below (tests/test_rtcp_cpu.py draws the same), over states of which some are crafted; REPORT is
 *       make_report, INPLACE 1 passes one array as state_in and state_out; every output printed as one line of numbers
 *   rtcp_plan_driver refuse
 *       the refusals in the header's order on a NULL batch, on a zero-filled block in place of a batch and on the host plan; every array is a block of 64 bytes */
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

static int stats(char** v)
{
    lcg_x = (uint32_t)atoi(v[0]);
    const int N = atoi(v[1]), S = atoi(v[2]), report = atoi(v[3]), inplace = atoi(v[4]);
    if (N < 1 || S < 1) return 2;
    const size_t n = (size_t)N, s = (size_t)S;
    int32_t* stream = block(4 * n); int32_t* seq = block(4 * n); int32_t* ts = block(4 * n); int32_t* arr = block(4 * n);
    int32_t* st_in = block(4 * s * LC3PLUS_RR_STATE_WORDS); int32_t* st_out = inplace ? st_in : block(4 * s * LC3PLUS_RR_STATE_WORDS);
    int32_t* ssrc = block(4 * s); int32_t* lsr = block(4 * s); int32_t* dlsr = block(4 * s);
    uint32_t* next = block(4 * s);
    for (int k = 0; k < S; k++) {
        next[k] = lcg() & 1 ? 65530u : lcg() & 0xFFFFu;
        ssrc[k] = (int32_t)(0x80000001u + (uint32_t)k * 0x3FFFFFFFu); lsr[k] = (int32_t)(lcg() * 2654435761u); dlsr[k] = (int32_t)lcg();
        int32_t* w = st_in + (size_t)k * LC3PLUS_RR_STATE_WORDS;
        memset(w, 0, 4 * LC3PLUS_RR_STATE_WORDS);
        if (k % 3 == 1) {                                            /* a source that has started, with words of every size */
            w[0] = 1; w[1] = (int32_t)(lcg() & 0xFFFFu); w[2] = (int32_t)((next[k] - 1u) & 0xFFFFu); w[3] = (int32_t)(((lcg() & 0xFFu) << 16) * (k % 2 ? 0x101u : 1u));
            w[4] = 65537; w[5] = (int32_t)(lcg() * 517u); w[6] = (int32_t)(lcg() * 3u); w[7] = (int32_t)(lcg() * 5u); w[8] = (int32_t)(lcg() * 2654435761u);
            w[9] = (int32_t)(lcg() & 0xFFFFFu);
        }
    }
    for (int i = 0; i < N; i++) {
        const uint32_t d = lcg();
        const int k = d % 23 == 0 ? -1 : d % 29 == 0 ? S : (int)((d >> 4) % (uint32_t)S);
        stream[i] = k;
        uint32_t q = lcg();
        if (k >= 0 && k < S) {
            const uint32_t e = lcg() % 40;
            if (e == 0) next[k] += 3000u + lcg() % 60000u;           /* a jump; its successor follows */
            else if (e == 1) next[k] -= 1u + lcg() % 3u;             /* a step back: duplicates and reordered packets */
            else if (e == 2) next[k] += 1u + lcg() % 5u;             /* losses */
            q = next[k]++ + ((lcg() & 1) << 16);
        }
        seq[i] = (int32_t)q;
        ts[i] = (int32_t)(q * 480u + 0xFFFF0000u);
        const uint32_t far = lcg() % 7 == 0 ? 0x80000000u : 0u;
        arr[i] = (int32_t)((uint32_t)ts[i] + far + lcg() % 1000u);
    }
    uint8_t* blocks = block(s * LC3PLUS_RR_BLOCK_BYTES); int32_t* ext = block(4 * n); uint8_t* status = block(n); int32_t* tally = block(4 * s * LC3PLUS_RR_STATS_WORDS);
    /* first with every optional array NULL, on copies of the state */
    int32_t* c_in = block(4 * s * LC3PLUS_RR_STATE_WORDS); int32_t* c_out = block(4 * s * LC3PLUS_RR_STATE_WORDS);
    memcpy(c_in, st_in, 4 * s * LC3PLUS_RR_STATE_WORDS);
    if (lc3plus_plan_rtcp_stats(N, stream, seq, ts, arr, S, c_in, c_out, report, report ? ssrc : NULL, NULL, NULL, report ? blocks : NULL, NULL, NULL, NULL)) return 1;
    const LC3_Error e = lc3plus_plan_rtcp_stats(N, stream, seq, ts, arr, S, st_in, st_out, report, ssrc, lsr, dlsr, blocks, ext, status, tally);
    printf("rc %d\n", (int)e);
    if (e) return 0;
    if (memcmp(c_out, st_out, 4 * s * LC3PLUS_RR_STATE_WORDS)) return 1;    /* the optional arrays change nothing of the state */
    PRINT("state", st_out, s * LC3PLUS_RR_STATE_WORDS, " %d", int); PRINT("blocks", blocks, s * LC3PLUS_RR_BLOCK_BYTES, " %d", int); PRINT("ext_seq", ext, N, " %d", int);
    PRINT("item_status", status, N, " %d", int); PRINT("stream_stats", tally, s * LC3PLUS_RR_STATS_WORDS, " %d", int);
    printf("workspace %lld\n", (long long)lc3plus_rtcp_workspace_bytes(N, S));
    free(stream); free(seq); free(ts); free(arr); if (!inplace) free(st_out);
    free(st_in); free(ssrc); free(lsr); free(dlsr); free(next); free(blocks); free(ext); free(status); free(tally); free(c_in); free(c_out);
    return 0;
}

#define WANT(x, code) do { const LC3_Error e_ = (x); if (e_ != (code)) { printf("%s: %d, not %d\n", #x, (int)e_, (int)(code)); return 1; } } while (0)
static int refuse(void)
{
    uint8_t* fake = calloc(1, 4096);                                 /* stands in for a batch: no refusal reads or writes it */
    int32_t* a = calloc(1, 64);
    if (!fake || !a) return 3;
    lc3plus_dec_batch* b = (lc3plus_dec_batch*)fake;
    uint8_t* a8 = (uint8_t*)a;
    const int64_t W = lc3plus_rtcp_workspace_bytes(1, 1);
    if (W <= 0 || lc3plus_rtcp_workspace_bytes(0, 1) || lc3plus_rtcp_workspace_bytes(1, 0) || lc3plus_rtcp_workspace_bytes(1LL << 29, 1) ||
        lc3plus_rtcp_workspace_bytes(-1, -1)) return 1;
    if (lc3plus_rtcp_workspace_bytes(1000000, 100) < 4 * 1000000LL) return 1;
#define CALL(bb, n, p0, p1, p2, p3, S, si, so, mr, sr, bl, w, wb) lc3plus_dec_batch_rtcp_stats(bb, n, p0, p1, p2, p3, S, si, so, mr, sr, NULL, NULL, bl, NULL, NULL, NULL, w, wb, NULL, 1)
    WANT(CALL(NULL, 1, a, a, a, a, 1, a, a, 0, NULL, NULL, a, W), LC3_NULL_ERROR);
    WANT(CALL(NULL, 0, NULL, a, a, a, 0, a, a, 7, NULL, NULL, NULL, 0), LC3_NULL_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 1, a, a, 0, NULL, NULL, NULL, W), LC3_NULL_ERROR);
    WANT(CALL(b, 1, NULL, a, a, a, 1, a, a, 0, NULL, NULL, a, W), LC3_NULL_ERROR);
    WANT(CALL(b, 1, a, NULL, a, a, 1, a, a, 0, NULL, NULL, a, W), LC3_NULL_ERROR);
    WANT(CALL(b, 1, a, a, NULL, a, 1, a, a, 0, NULL, NULL, a, W), LC3_NULL_ERROR);
    WANT(CALL(b, 1, a, a, a, NULL, 1, a, a, 0, NULL, NULL, a, W), LC3_NULL_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 1, NULL, a, 0, NULL, NULL, a, W), LC3_NULL_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 1, a, NULL, 0, NULL, NULL, a, W), LC3_NULL_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 1, a, a, 1, NULL, a8, a, W), LC3_NULL_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 1, a, a, 1, a, NULL, a, W), LC3_NULL_ERROR);
    WANT(CALL(b, 0, a, a, a, a, 0, a, NULL, 0, NULL, NULL, a, 0), LC3_NULL_ERROR);                    /* NULL first */
    WANT(CALL(b, 0, a, a, a, a, 1, a, a, 0, NULL, NULL, a, W), LC3_ERROR);
    WANT(CALL(b, -1, a, a, a, a, 1, a, a, 0, NULL, NULL, a, W), LC3_ERROR);
    WANT(CALL(b, 1LL << 29, a, a, a, a, 1, a, a, 0, NULL, NULL, a, INT64_MAX), LC3_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 0, a, a, 0, NULL, NULL, a, W), LC3_ERROR);
    WANT(CALL(b, 1, a, a, a, a, -3, a, a, 0, NULL, NULL, a, W), LC3_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 1, a, a, 2, a, a8, a, W), LC3_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 1, a, a, -1, a, a8, a, W), LC3_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 1, a, a, 0, NULL, NULL, a, W - 1), LC3_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 1, a, a, 1, a, a8, a, 0), LC3_ERROR);
    WANT(CALL(b, 1, a, a, a, a, 1, a, a, 0, NULL, NULL, a, W), LC3_ERROR);                            /* every check passed: no device behind the stub */
#define PLAN(n, p0, S, si, so, mr, sr, bl) lc3plus_plan_rtcp_stats(n, p0, a, a, a, S, si, so, mr, sr, NULL, NULL, bl, NULL, NULL, NULL)
    WANT(PLAN(1, NULL, 1, a, a, 0, NULL, NULL), LC3_NULL_ERROR);
    WANT(PLAN(1, a, 1, NULL, a, 0, NULL, NULL), LC3_NULL_ERROR);
    WANT(PLAN(1, a, 1, a, NULL, 0, NULL, NULL), LC3_NULL_ERROR);
    WANT(PLAN(1, a, 1, a, a, 1, NULL, a8), LC3_NULL_ERROR);
    WANT(PLAN(1, a, 1, a, a, 1, a, NULL), LC3_NULL_ERROR);
    WANT(PLAN(0, a, 1, a, a, 0, NULL, NULL), LC3_ERROR);
    WANT(PLAN(1, a, 0, a, a, 0, NULL, NULL), LC3_ERROR);
    WANT(PLAN(1, a, 1, a, a, 3, a, a8), LC3_ERROR);
    for (int k = 0; k < 4096; k++) if (fake[k]) { printf("the batch was written at byte %d\n", k); return 1; }
    for (int k = 0; k < 64; k++) if (a8[k]) { printf("an array was written at byte %d\n", k); return 1; }
    free(fake); free(a);
    printf("refusals ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 7 && !strcmp(argv[1], "stats")) return stats(argv + 2);
    if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse();
    fprintf(stderr, "usage: rtcp_plan_driver stats SEED N S REPORT INPLACE | refuse\n");
    return 2;
}
