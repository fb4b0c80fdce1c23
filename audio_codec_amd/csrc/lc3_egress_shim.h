/* lc3_egress_shim.h -- packet egress (include/lc3plus_batch.h "Packet egress": lc3plus_enc_batch_egress, lc3plus_dec_batch_egress, lc3plus_plan_egress): what the
 * host C code (lc3_packet.c) and the sibling library that holds the egress kernels (lc3_egress.hip -> liblc3plus_egress_hip.so) share.  The route rule, the cell
 * rule, the sequence numbers, the packet's advance in the wire buffer and the packet record are one text for the host function and the kernels; the
 * lc3egress_* functions are the sibling's whole C ABI.  lc3_packet.c loads the sibling from its own directory on the first egress call; the code objects of the
 * other libraries hold none of this. */
#ifndef LC3_EGRESS_SHIM_H
#define LC3_EGRESS_SHIM_H
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC3E_HD __host__ __device__
#else
#define LC3E_HD
#endif

/* LC3PLUS_EGR_* of include/lc3plus_batch.h: a cell's status, a packet's flags, the words of a route's stats */
enum { LC3E_SENT = 1, LC3E_LOST = 2, LC3E_INVALID = 4, LC3E_SKIPPED = 8, LC3E_ABSENT = 16, LC3E_BAD_ROUTE = 32, LC3E_OVERFLOW = 64 };
enum { LC3E_PKT_OVERFLOW = 1 };
enum { LC3E_STATS_WORDS = 4, LC3E_ST_COUNT = 0, LC3E_ST_SENT = 1, LC3E_ST_HOLES = 2, LC3E_ST_OVERFLOW = 3 };
enum { LC3E_STREAM_MAJOR = 0, LC3E_FRAME_MAJOR = 1 };
/* the scan runs over tiles of LC3E_TILE cells: LC3E_THREADS lanes with LC3E_ITEMS neighbouring cells each.  n_routes * n_frames < LC3E_MAX_CELLS */
enum { LC3E_THREADS = 256, LC3E_ITEMS = 4, LC3E_TILE = LC3E_THREADS * LC3E_ITEMS };
#define LC3E_MAX_CELLS (1LL << 31)
#define LC3E_MAX_ALIGN 4096

/* The workspace of a call, in this order: word [n_cells] int32, one per cell in list order (a SENT cell's frame size, else minus its status); the tiles' sums
 * and then bases [n_tiles][2] int64 {packets, bytes}; status [n_cells] uint8 by (route, frame), used where the caller gives no cell_status but wants stats;
 * from [n_cells] int64, each packet's source offset for the copy (wire mode). */
static inline LC3E_HD long long lc3e_tiles(long long n_cells) { return (n_cells + LC3E_TILE - 1) / LC3E_TILE; }
static inline LC3E_HD long long lc3e_work_sums(long long n_cells) { return (4 * n_cells + 7) & ~7LL; }
static inline LC3E_HD long long lc3e_work_status(long long n_cells) { return lc3e_work_sums(n_cells) + 16 * lc3e_tiles(n_cells); }
static inline LC3E_HD long long lc3e_work_from(long long n_cells) { return lc3e_work_status(n_cells) + ((n_cells + 7) & ~7LL); }
static inline LC3E_HD long long lc3e_work_bytes(long long n_cells) { return lc3e_work_from(n_cells) + 8 * n_cells; }

/* cell i of the list order -> its route and frame: stream-major i = r n_frames + t, frame-major i = t n_routes + r */
static inline LC3E_HD void lc3e_cell_rt(long long i, int n_routes, int n_frames, int order, int* r, int* t)
{
    if (order == LC3E_FRAME_MAJOR) { *t = (int)(i / n_routes); *r = (int)(i - (long long)*t * n_routes); }
    else { *r = (int)(i / n_frames); *t = (int)(i - (long long)*r * n_frames); }
}
/* The route rule: -> the frames route r sends from (its source's count clamped to the call), its source in *s; -1 for a route whose source is no stream */
static inline LC3E_HD int lc3e_route(const int32_t* route_src, int r, int n_streams, const int32_t* counts, int n_frames, int* s)
{
    const int src = route_src ? route_src[r] : r;
    if (src < 0 || src >= n_streams) return -1;
    *s = src;
    const int c = counts ? counts[src] : n_frames;
    return c < 0 ? 0 : c > n_frames ? n_frames : c;
}
/* The cell rule for a cell in front of its route's count: LOST, INVALID, SKIPPED or SENT from the frame's size, offset and flag byte, in that order */
static inline LC3E_HD int lc3e_class(int32_t nb, long long off, int flag, int max_frame_bytes, long long capacity, int skip_mask)
{
    if (nb == 0) return LC3E_LOST;
    if (nb < 0 || nb > max_frame_bytes || off < 0 || off > capacity - nb) return LC3E_INVALID;      /* capacity >= 0 and nb > 0: no overflow */
    if (flag & skip_mask) return LC3E_SKIPPED;
    return LC3E_SENT;
}
/* a cell's word of the workspace: its frame's size (> 0) where it is SENT, minus its status otherwise.  Nothing of an ABSENT or BAD_ROUTE cell's tables is read */
static inline LC3E_HD int32_t lc3e_cell_word(int r, int t, int n_streams, const int32_t* route_src, const int32_t* counts, int n_frames, const long long* offsets,
                                             const int32_t* num_bytes, const uint8_t* flags, int max_frame_bytes, long long capacity, int skip_mask)
{
    int s = 0;
    const int c = lc3e_route(route_src, r, n_streams, counts, n_frames, &s);
    if (c < 0) return -LC3E_BAD_ROUTE;
    if (t >= c) return -LC3E_ABSENT;
    const size_t k = (size_t)s * n_frames + t;
    const int32_t nb = num_bytes[k];
    const int cls = lc3e_class(nb, nb ? offsets[k] : 0, nb && flags ? flags[k] : 0, max_frame_bytes, capacity, skip_mask);
    return cls == LC3E_SENT ? nb : -cls;
}
/* what a cell of that word adds to the running byte offset: in place its frame's size, in wire mode header_room + size rounded up to align; 0 unless SENT */
static inline LC3E_HD long long lc3e_advance(int32_t word, int wire_mode, int header_room, int align)
{
    if (word <= 0) return 0;
    return wire_mode ? ((long long)header_room + word + align - 1) & ~(long long)(align - 1) : word;
}
/* (base + t) mod 2^seq_bits, seq_bits 16 or 32 */
static inline LC3E_HD int32_t lc3e_seq(int32_t base, int t, int seq_bits)
{
    const uint32_t u = (uint32_t)base + (uint32_t)t;
    return seq_bits == 16 ? (int32_t)(u & 0xFFFFu) : (int32_t)u;
}
static inline LC3E_HD int lc3e_fits(long long off, int32_t pkt_size, int wire_mode, long long wire_capacity) { return !wire_mode || off <= wire_capacity - pkt_size; }

/* the list arrays and the per-cell status of one call; from: each packet's source offset (the workspace's, wire mode) or NULL */
typedef struct { int32_t* route; int32_t* seq; int32_t* frame; long long* offset; int32_t* size; uint8_t* flags; uint8_t* status; long long* from; } lc3e_list;
/* The packet record of a SENT cell (r, t) of source s with frame size nb: list entry p at running offset run.  -> the cell's status */
static inline LC3E_HD int lc3e_emit(const lc3e_list* L, long long p, int r, int t, int s, int32_t nb, long long run, const int32_t* seq_base, int seq_bits, int n_frames,
                                    const long long* offsets, int wire_mode, int header_room, long long wire_capacity)
{
    const int32_t size = header_room + nb;
    const long long src = offsets[(size_t)s * n_frames + t];
    const long long off = wire_mode ? run : src;
    const int fit = lc3e_fits(off, size, wire_mode, wire_capacity);
    L->route[p] = r; L->seq[p] = lc3e_seq(seq_base[r], t, seq_bits); L->frame[p] = t; L->offset[p] = off; L->size[p] = size;
    if (L->flags) L->flags[p] = (uint8_t)(fit ? 0 : LC3E_PKT_OVERFLOW);
    if (L->from) L->from[p] = src;
    return LC3E_SENT | (fit ? 0 : LC3E_OVERFLOW);
}
/* a route's stats and next sequence number from its count c (-1: a bad route) and its cells' tallies */
static inline LC3E_HD void lc3e_route_out(int r, int c, int sent, int holes, int over, const int32_t* seq_base, int seq_bits, int32_t* next_seq, int32_t* stats)
{
    if (next_seq) next_seq[r] = c < 0 ? seq_base[r] : lc3e_seq(seq_base[r], c, seq_bits);
    if (stats) {
        int32_t* q = stats + (size_t)r * LC3E_STATS_WORDS;
        q[LC3E_ST_COUNT] = c < 0 ? 0 : c; q[LC3E_ST_SENT] = sent; q[LC3E_ST_HOLES] = holes; q[LC3E_ST_OVERFLOW] = over;
    }
}
/* The copy rule.  A frame of n bytes goes to byte address dst in the widest pieces dst allows: hb head bytes up to its first 4-byte boundary, hd head words up
 * to its first 16-byte boundary, `pieces` pieces of 16 bytes, then td tail words and tb tail bytes - each run cut short where the frame ends first.  Of the
 * source only aligned 32-bit words that hold a byte of the frame are read. */
typedef struct { int hb, hd, pieces, td, tb; } lc3e_copy_plan;
static inline LC3E_HD lc3e_copy_plan lc3e_copy_layout(uintptr_t dst, int n)
{
    lc3e_copy_plan c;
    const int hb = (int)((0 - dst) & 3);
    c.hb = hb < n ? hb : n;
    n -= c.hb;
    const int hd = (int)((0 - (dst + (uintptr_t)c.hb)) & 15) >> 2;
    c.hd = hd < (n >> 2) ? hd : n >> 2;
    n -= 4 * c.hd;
    c.pieces = n >> 4; c.td = (n & 15) >> 2; c.tb = n & 3;
    return c;
}

/* one egress call: every pointer but the struct itself is a device pointer (those that may be NULL: flags, counts, route_src, wire, pkt_flags, wire_total, next_seq,
 * stats, cell_status) */
typedef struct {
    int32_t device, n_streams, n_frames, max_frame_bytes, skip_mask, n_routes, seq_bits, order, header_room, align, sync;
    long long frames_capacity, wire_capacity;
    const void* frames; const long long* offsets; const int32_t* num_bytes; const uint8_t* flags; const int32_t* counts; const int32_t* route_src; const int32_t* seq_base;
    void* wire;
    lc3e_list list;
    long long* n_packets; long long* wire_total; int32_t* next_seq; int32_t* stats;
    void* work; void* hip_stream;
} lc3egress_call;

#ifdef __cplusplus
extern "C" {
#endif
/* queues the egress kernels on q->hip_stream; waits for them only with q->sync.  0, or 1 where nothing was queued */
int lc3egress_run(const lc3egress_call* q);
/* launches of an egress kernel by this process, by the kernel's symbol name in the code object; -1 for a name the library does not hold */
long long lc3egress_launch_count(const char* kernel);
#ifdef __cplusplus
}
#endif
#endif
