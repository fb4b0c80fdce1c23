/* lc3_rtcp_shim.h -- reception reports (include/lc3plus_batch.h "Reception reports": lc3plus_dec_batch_rtcp_stats, lc3plus_plan_rtcp_stats,
 * lc3plus_rtcp_workspace_bytes): what the host C code (lc3_packet.c) and the sibling library that holds the kernels (lc3_rtcp.hip -> liblc3plus_rtcp_hip.so)
 * share.  The rule of one item (RFC 3550 A.1 without probation, A.8), the rule of one report (A.3), the block's words and the workspace's layout are one text
 * for the host function and the kernels.  The lc3rtcp_* functions are the sibling's whole C ABI.  lc3_packet.c loads the sibling from its own directory on the
 * first call; the code objects of the other libraries hold none of this. */
#ifndef LC3_RTCP_SHIM_H
#define LC3_RTCP_SHIM_H
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC3Q_HD __host__ __device__
#else
#define LC3Q_HD
#endif

/* LC3PLUS_RR_* of include/lc3plus_batch.h: the words of a stream's state, an item's status, the words of a stream's stats */
enum { LC3Q_FLAGS = 0, LC3Q_BASE_SEQ = 1, LC3Q_MAX_SEQ = 2, LC3Q_CYCLES = 3, LC3Q_BAD_SEQ = 4, LC3Q_RECEIVED = 5, LC3Q_EXPECTED_PRIOR = 6, LC3Q_RECEIVED_PRIOR = 7,
       LC3Q_TRANSIT = 8, LC3Q_JITTER = 9, LC3Q_STATE_WORDS = 10 };
enum { LC3Q_STARTED = 1 };
enum { LC3Q_DROPPED = 0, LC3Q_COUNTED = 1, LC3Q_JUMP = 2, LC3Q_RESTART = 3, LC3Q_REORDERED = 4 };
enum { LC3Q_ST_COUNTED = 0, LC3Q_ST_JUMP = 1, LC3Q_ST_RESTART = 2, LC3Q_ST_REORDERED = 3, LC3Q_STATS_WORDS = 4 };
/* RFC 3550 A.1: MAX_DROPOUT, MAX_MISORDER, RTP_SEQ_MOD */
enum { LC3Q_MAX_DROPOUT = 3000, LC3Q_MAX_MISORDER = 100, LC3Q_SEQ_MOD = 65536, LC3Q_BLOCK_BYTES = 24, LC3Q_BLOCK_WORDS = 6 };
#define LC3Q_MAX_ITEMS (1LL << 29)
/* The walk kernel sorts a stream's item indices in registers up to LC3Q_WAVE_ITEMS and in its workgroup's LDS (4 KiB) up to LC3Q_LDS_ITEMS; a longer segment
 * is placed in order by the place kernel and walked where it lies, in the workspace */
enum { LC3Q_THREADS = 256, LC3Q_WALK_THREADS = 64, LC3Q_WAVE_ITEMS = 64, LC3Q_LDS_ITEMS = 1024, LC3Q_SCAN_THREADS = 1024, LC3Q_PLACE_THREADS = 1024 };

typedef struct { uint32_t w[LC3Q_STATE_WORDS]; } lc3q_state;

/* ---- the rule of one item (rules 2 to 4) ---- */
static inline LC3Q_HD void lc3q_init_seq(lc3q_state* s, uint32_t q)
{
    s->w[LC3Q_BASE_SEQ] = q; s->w[LC3Q_MAX_SEQ] = q; s->w[LC3Q_BAD_SEQ] = LC3Q_SEQ_MOD + 1;
    s->w[LC3Q_CYCLES] = 0; s->w[LC3Q_RECEIVED] = 0; s->w[LC3Q_RECEIVED_PRIOR] = 0; s->w[LC3Q_EXPECTED_PRIOR] = 0;
    s->w[LC3Q_FLAGS] |= LC3Q_STARTED;
}
/* an item of a valid stream with sequence number seq and transit = arrival - timestamp: -> its status; *ext: its ext_seq */
static inline LC3Q_HD int lc3q_step(lc3q_state* s, uint32_t seq, uint32_t transit, uint32_t* ext)
{
    const uint32_t q = seq & 0xFFFFu;
    int first = 0, st = LC3Q_COUNTED;
    *ext = 0;
    if (!(s->w[LC3Q_FLAGS] & LC3Q_STARTED)) { lc3q_init_seq(s, q); first = 1; }
    else {
        const uint32_t udelta = (q - s->w[LC3Q_MAX_SEQ]) & 0xFFFFu;
        if (udelta < LC3Q_MAX_DROPOUT) {
            if (q < s->w[LC3Q_MAX_SEQ]) s->w[LC3Q_CYCLES] += LC3Q_SEQ_MOD;
            s->w[LC3Q_MAX_SEQ] = q;
        } else if (udelta <= LC3Q_SEQ_MOD - LC3Q_MAX_MISORDER) {
            if (q != s->w[LC3Q_BAD_SEQ]) { s->w[LC3Q_BAD_SEQ] = (q + 1) & 0xFFFFu; return LC3Q_JUMP; }
            lc3q_init_seq(s, q); first = 1; st = LC3Q_RESTART;
        } else st = LC3Q_REORDERED;
    }
    s->w[LC3Q_RECEIVED] += 1;
    if (first) { s->w[LC3Q_TRANSIT] = transit; s->w[LC3Q_JITTER] = 0; }
    else {
        const uint32_t d = transit - s->w[LC3Q_TRANSIT];
        s->w[LC3Q_TRANSIT] = transit;
        const uint32_t ad = (int32_t)d < 0 ? 0u - d : d;
        s->w[LC3Q_JITTER] += ad - ((s->w[LC3Q_JITTER] + 8u) >> 4);
    }
    *ext = s->w[LC3Q_CYCLES] + q - (q > s->w[LC3Q_MAX_SEQ] ? (uint32_t)LC3Q_SEQ_MOD : 0u);
    return st;
}

/* ---- the rule of one report (rule 6) ---- */
static inline LC3Q_HD uint32_t lc3q_be32(uint32_t v) { return v >> 24 | (v >> 16 & 255u) << 8 | (v >> 8 & 255u) << 16 | (v & 255u) << 24; }
/* a stream's block as six words (blk[k] holds bytes 4k .. 4k + 3 of the block, byte 4k lowest: stored as little-endian words they are the block), and the
 * priors advanced */
static inline LC3Q_HD void lc3q_report(lc3q_state* s, uint32_t ssrc, uint32_t lsr, uint32_t dlsr, uint32_t blk[LC3Q_BLOCK_WORDS])
{
    if (!(s->w[LC3Q_FLAGS] & LC3Q_STARTED)) { for (int k = 0; k < LC3Q_BLOCK_WORDS; k++) blk[k] = 0; return; }
    const uint32_t expected = s->w[LC3Q_CYCLES] + s->w[LC3Q_MAX_SEQ] - s->w[LC3Q_BASE_SEQ] + 1u;
    int32_t lost = (int32_t)(expected - s->w[LC3Q_RECEIVED]);
    lost = lost < -0x800000 ? -0x800000 : lost > 0x7FFFFF ? 0x7FFFFF : lost;
    const uint32_t uei = expected - s->w[LC3Q_EXPECTED_PRIOR], uri = s->w[LC3Q_RECEIVED] - s->w[LC3Q_RECEIVED_PRIOR];
    const int32_t ei = (int32_t)uei, li = (int32_t)(uei - uri);
    long long fraction = 0;
    if (ei != 0 && li > 0) { fraction = ((long long)li * 256) / ei; if (fraction > 255) fraction = 255; }
    s->w[LC3Q_EXPECTED_PRIOR] = expected; s->w[LC3Q_RECEIVED_PRIOR] = s->w[LC3Q_RECEIVED];
    blk[0] = lc3q_be32(ssrc);
    blk[1] = lc3q_be32(((uint32_t)fraction & 255u) << 24 | ((uint32_t)lost & 0xFFFFFFu));
    blk[2] = lc3q_be32(s->w[LC3Q_CYCLES] + s->w[LC3Q_MAX_SEQ]);
    blk[3] = lc3q_be32(s->w[LC3Q_JITTER] >> 4);
    blk[4] = lc3q_be32(lsr);
    blk[5] = lc3q_be32(dlsr);
}
/* the block's 24 bytes: six word stores where the address is 4-aligned, byte stores otherwise */
static inline LC3Q_HD void lc3q_block_out(uint8_t* d, const uint32_t blk[LC3Q_BLOCK_WORDS])
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (!((uintptr_t)d & 3)) { uint32_t* d4 = (uint32_t*)d; for (int k = 0; k < LC3Q_BLOCK_WORDS; k++) d4[k] = blk[k]; return; }
#endif
    for (int k = 0; k < LC3Q_BLOCK_BYTES; k++) d[k] = (uint8_t)(blk[k >> 2] >> ((k & 3) * 8));
}

/* ---- the workspace ---- */
/* int32 words behind the workspace's first 16-aligned byte: off [n_streams + 1] (each stream's first place in idx; the last is the number of placed items), cur
 * [n_streams] (the count kernel's counts, then the scatter's cursors), nbig [1] and big [most_big] (the streams with more than LC3Q_LDS_ITEMS items), idx
 * [n_items] (the item indices, stream by stream) */
static inline LC3Q_HD long long lc3q_most_big(long long n_items, long long n_streams)
{
    const long long m = n_items / (LC3Q_LDS_ITEMS + 1);
    return m < n_streams ? m : n_streams;
}
static inline LC3Q_HD long long lc3q_workspace_bytes(long long n_items, long long n_streams)
{
    if (n_items <= 0 || n_items >= LC3Q_MAX_ITEMS || n_streams <= 0) return 0;
    return 16 + 4 * ((n_streams + 1) + n_streams + 1 + lc3q_most_big(n_items, n_streams) + n_items);
}

/* one call: every pointer but the struct itself is a device pointer (those that may be NULL: lsr, dlsr, ext_seq, item_status, stream_stats; without make_report
 * also ssrc and blocks) */
typedef struct {
    int32_t device, n_streams, make_report, sync;
    long long n_items;
    const int32_t* stream; const int32_t* seq; const int32_t* timestamp; const int32_t* arrival;
    const int32_t* state_in; int32_t* state_out;
    const int32_t* ssrc; const int32_t* lsr; const int32_t* dlsr; uint8_t* blocks;
    int32_t* ext_seq; uint8_t* item_status; int32_t* stream_stats;
    void* workspace; long long workspace_bytes;
    void* hip_stream;
} lc3rtcp_stats_call;

#ifdef __cplusplus
extern "C" {
#endif
/* queue the kernels on q->hip_stream; wait for them only with q->sync.  0, or 1 where nothing was queued */
int lc3rtcp_stats_run(const lc3rtcp_stats_call* q);
/* launches of a kernel of this library by this process, by the kernel's symbol name in the code object; -1 for a name the library does not hold */
long long lc3rtcp_launch_count(const char* kernel);
#ifdef __cplusplus
}
#endif
#endif
