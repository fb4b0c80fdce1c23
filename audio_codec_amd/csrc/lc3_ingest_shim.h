/* lc3_ingest_shim.h -- packet ingest (include/lc3plus_batch.h "Packet ingest": lc3plus_dec_batch_ingest, lc3plus_plan_ingest): what the host C code (lc3_packet.c)
 * and the sibling library that holds the ingest kernels (lc3_ingest.hip -> liblc3plus_ingest_hip.so) share.  The item rule, the cell key and the per-stream
 * count are one text for the host function and the kernels; the lc3ingest_* functions are the sibling's whole C ABI.  lc3_packet.c loads the sibling from its own
 * directory on the first ingest call; neither the codec library's nor the probe library's code object holds any of this. */
#ifndef LC3_INGEST_SHIM_H
#define LC3_INGEST_SHIM_H
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC3I_HD __host__ __device__
#else
#define LC3I_HD
#endif

/* LC3PLUS_ING_* of include/lc3plus_batch.h */
enum { LC3I_USED = 1, LC3I_DUPLICATE = 2, LC3I_LATE = 4, LC3I_EARLY = 8, LC3I_BAD_STREAM = 16, LC3I_EMPTY = 32, LC3I_REFUSED = 64, LC3I_INVALID = 128 };
enum { LC3I_STATS_WORDS = 4, LC3I_ST_COUNT = 0, LC3I_ST_GAPS = 1, LC3I_ST_LATE = 2, LC3I_ST_EARLY = 3 };
/* of a probe record (lc3_probe_shim.h) the ingest reads the status word alone */
enum { LC3I_INFO_WORDS = 48, LC3I_FI_INVALID = 2, LC3I_FI_LOST = 4 };
/* a cell's key while the items are sorted in: rank << LC3I_RANK_SHIFT | item, the smallest wins; all ones = no candidate yet.  n_items < LC3I_MAX_ITEMS */
#define LC3I_RANK_SHIFT 29
#define LC3I_MAX_ITEMS  (1LL << LC3I_RANK_SHIFT)
#define LC3I_NO_KEY     0xFFFFFFFFu
#define LC3I_ITEM_MASK  ((1u << LC3I_RANK_SHIFT) - 1u)

/* the slot distance of a sequence number from its stream's base: the difference mod 2^seq_bits, sign-extended (seq_bits 16 or 32) */
static inline LC3I_HD int32_t lc3i_distance(int32_t seq, int32_t base, int seq_bits)
{
    const uint32_t u = (uint32_t)seq - (uint32_t)base;
    return seq_bits == 16 ? (int32_t)(int16_t)(uint16_t)u : (int32_t)u;
}
/* The item rule.  rec: the item's probe records [channels][LC3I_INFO_WORDS] or NULL; base: [n_streams].  -> LC3I_BAD_STREAM, _EMPTY, _LATE or _EARLY, or 0 for a
 * candidate: then *t is its frame and *rank 0 (the decoder decodes it), 1 (refused by the bitstream checks) or 2 (invalid) */
static inline LC3I_HD int lc3i_item(int32_t s, int32_t seq, int32_t nb, const int32_t* rec, int channels, int n_streams, const int32_t* base, int seq_bits,
                                    int n_frames, int* t, int* rank)
{
    if (s < 0 || s >= n_streams) return LC3I_BAD_STREAM;
    int any = 0, all = 0;
    if (rec)
        for (int ch = 0; ch < channels; ch++) { const int st = rec[(size_t)ch * LC3I_INFO_WORDS]; any |= st != 0; all |= st; }
    if (nb == 0 || (all & LC3I_FI_LOST)) return LC3I_EMPTY;
    const int32_t d = lc3i_distance(seq, base[s], seq_bits);
    if (d < 0) return LC3I_LATE;
    if (d >= n_frames) return LC3I_EARLY;
    *t = d;
    *rank = !any ? 0 : (all & LC3I_FI_INVALID) ? 2 : 1;
    return 0;
}
static inline LC3I_HD uint32_t lc3i_key(int rank, long long item) { return ((uint32_t)rank << LC3I_RANK_SHIFT) | (uint32_t)item; }
/* the status byte of a candidate of that rank for a cell that item `winner` won */
static inline LC3I_HD int lc3i_candidate_status(int rank, long long item, int32_t winner)
{
    return (item == winner ? LC3I_USED : LC3I_DUPLICATE) | (rank == 1 ? LC3I_REFUSED : rank == 2 ? LC3I_INVALID : 0);
}
/* frames a stream advances by: its floor (or NULL's 0) clamped to the call, or up to its last filled cell (top: the highest t with a winner, -1 for none) */
static inline LC3I_HD int lc3i_count(int floor_s, int n_frames, int top)
{
    const int f = floor_s < 0 ? 0 : floor_s > n_frames ? n_frames : floor_s;
    return f > top + 1 ? f : top + 1;
}
static inline LC3I_HD int32_t lc3i_next_base(int32_t base, int count, int seq_bits)
{
    const uint32_t u = (uint32_t)base + (uint32_t)count;
    return seq_bits == 16 ? (int32_t)(u & 0xFFFFu) : (int32_t)u;
}

/* one ingest call: every pointer but the struct itself is a device pointer (those that may be NULL: info, floor, next_base, stats, item_status) */
typedef struct {
    int32_t device, n_streams, channels, seq_bits, n_frames, sync;
    long long n_items;
    const int32_t* stream; const int32_t* seq; const long long* offsets; const int32_t* num_bytes; const int32_t* info; const int32_t* base; const int32_t* floor;
    long long* out_offsets; int32_t* out_num_bytes; int32_t* cell_item; int32_t* counts; int32_t* next_base; int32_t* stats; uint8_t* item_status;
    void* hip_stream;
} lc3ingest_call;

#ifdef __cplusplus
extern "C" {
#endif
/* queues the ingest kernels on q->hip_stream; waits for them only with q->sync.  0, or 1 where nothing was queued */
int lc3ingest_run(const lc3ingest_call* q);
/* launches of an ingest kernel by this process, by the kernel's symbol name in the code object; -1 for a name the library does not hold */
long long lc3ingest_launch_count(const char* kernel);
#ifdef __cplusplus
}
#endif
#endif
