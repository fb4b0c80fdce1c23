/* lc3_red_shim.h -- redundant audio, RFC 2198 (include/lc3plus_batch.h "Redundant audio": lc3plus_{enc,dec}_batch_red_pack, lc3plus_dec_batch_red_unpack,
 * lc3plus_plan_red_pack, lc3plus_plan_red_unpack): what the host C code (lc3_packet.c) and the sibling library that holds the RED kernels (lc3_red.hip ->
 * liblc3plus_red_hip.so) share.  The packet rule, the block header's bytes, the tail rule, the workspace's layout and the unpack rule are one text for the host
 * functions and the kernels; they differ only in how a payload's bytes are fetched (plain bytes on the host, aligned 32-bit words realigned in registers on the
 * device, the idiom of lc3_rtp_shim.h).  The route rule, the cell rule and the copy rule are the egress's (lc3_egress_shim.h), by inclusion.  The lc3red_*
 * functions are the sibling's whole C ABI.  lc3_packet.c loads the sibling from its own directory on the first RED call; the code objects of the other libraries
 * hold none of this. */
#ifndef LC3_RED_SHIM_H
#define LC3_RED_SHIM_H
#include <stdint.h>
#include <stddef.h>
#include "lc3_egress_shim.h"
#include "lc3_rtp_shim.h"

#define LC3RED_HD LC3E_HD

/* LC3PLUS_RED_* of include/lc3plus_batch.h */
enum { LC3RED_MAX_DEPTH = 4, LC3RED_MAX_BLOCK = 1023, LC3RED_MAX_TS_OFFSET = 16383, LC3RED_PKT_BAD = 2 };
enum { LC3RED_RS_WORDS = 4, LC3RED_RS_PACKETS = 0, LC3RED_RS_BLOCKS = 1, LC3RED_RS_BLOCK_BYTES = 2, LC3RED_RS_MISSED = 3 };
enum { LC3RED_OK = 0, LC3RED_DROPPED = 1, LC3RED_RANGE = 2, LC3RED_SHORT = 3, LC3RED_DEPTH = 4, LC3RED_LENGTH = 5, LC3RED_PAYLOAD_TYPE = 6, LC3RED_STATUSES = 8,
       LC3RED_ST_DROP_TYPE = 8, LC3RED_ST_DROP_OFFSET = 9, LC3RED_ST_DROP_EMPTY = 10, LC3RED_TALLIES = 11, LC3RED_STATS_WORDS = 16 };
/* the scan runs over tiles of LC3RED_TILE packets: LC3RED_THREADS lanes with LC3RED_ITEMS neighbouring packets each; LC3RED_COPY_LANES lanes copy a packet */
enum { LC3RED_THREADS = 256, LC3RED_ITEMS = 4, LC3RED_TILE = LC3RED_THREADS * LC3RED_ITEMS, LC3RED_COPY_LANES = 8 };
#define LC3RED_MAX_PACKETS (1LL << 31)
/* the largest payload in front of the primary: four headers and the final byte, four blocks */
#define LC3RED_MAX_EXTRA (4 * LC3RED_MAX_DEPTH + 1 + LC3RED_MAX_DEPTH * LC3RED_MAX_BLOCK)

/* The workspace of a pack call, in this order: size [max_packets] int32, one per list entry (the packet's red_size, 0 for a BAD one); the tiles' sums and then
 * bases [n_tiles] int64; mask [max_packets] uint8 (bits 0 .. 3 the carried generations, bits 4 .. 6 the generations that existed and were not carried). */
static inline LC3RED_HD long long lc3red_tiles(long long max_packets) { return (max_packets + LC3RED_TILE - 1) / LC3RED_TILE; }
static inline LC3RED_HD long long lc3red_work_sums(long long max_packets) { return (4 * max_packets + 7) & ~7LL; }
static inline LC3RED_HD long long lc3red_work_mask(long long max_packets) { return lc3red_work_sums(max_packets) + 8 * lc3red_tiles(max_packets); }
static inline LC3RED_HD long long lc3red_work_bytes(long long max_packets) { return lc3red_work_mask(max_packets) + ((max_packets + 7) & ~7LL); }

/* ---- the pack rule ---- */
/* what a pack call reads (may be NULL: flags, counts, route_src, depth, tail_bytes, tail_sizes) */
typedef struct {
    const void* frames; const long long* offsets; const int32_t* num_bytes; const uint8_t* flags; const int32_t* counts; const int32_t* route_src;
    const int32_t* pkt_route; const int32_t* pkt_frame; const int32_t* depth; const int32_t* block_pt; const uint8_t* tail_bytes; const int32_t* tail_sizes;
    long long frames_capacity, wire_capacity;
    int32_t n_streams, n_frames, max_frame_bytes, skip_mask, n_routes, max_depth, ts_step, max_packet_bytes, tail_stride, header_room, align;
} lc3red_pack_in;
/* the list's length as every kernel reads it: *n_packets clamped to [0, max_packets] */
static inline LC3RED_HD long long lc3red_count(const long long* n_packets, long long max_packets)
{
    const long long n = *n_packets;
    return n < 0 ? 0 : n > max_packets ? max_packets : n;
}
/* a tail entry's size as given -> the size the rule takes: 0 (none) unless it lies in 1 ... min(1023, tail_stride) */
static inline LC3RED_HD int32_t lc3red_tail_size(int32_t v, int tail_stride) { return v > 0 && v <= LC3RED_MAX_BLOCK && v <= tail_stride ? v : 0; }
/* Frame u of stream s as a redundant block: -> its size and its address in *src, 0 where it does not exist.  u >= 0: frame (s, u) of the tables where its
 * class is SENT; u < 0: entry -u - 1 of the stream's tail where a tail is given and holds one */
static inline LC3RED_HD int32_t lc3red_block(const lc3red_pack_in* q, int s, int u, uintptr_t* src)
{
    if (u >= 0) {
        const size_t k = (size_t)s * q->n_frames + u;
        const int32_t nb = q->num_bytes[k];
        if (lc3e_class(nb, nb ? q->offsets[k] : 0, nb && q->flags ? q->flags[k] : 0, q->max_frame_bytes, q->frames_capacity, q->skip_mask) != LC3E_SENT) return 0;
        *src = (uintptr_t)q->frames + (uintptr_t)q->offsets[k];
        return nb;
    }
    const int g = -u - 1;
    if (!q->tail_sizes || g >= q->max_depth) return 0;
    const size_t e = (size_t)s * q->max_depth + g;
    *src = (uintptr_t)q->tail_bytes + e * (size_t)q->tail_stride;
    return lc3red_tail_size(q->tail_sizes[e], q->tail_stride);
}
/* a route's depth: depth[r] clamped to [0, max_depth], max_depth without the array */
static inline LC3RED_HD int lc3red_depth(const lc3red_pack_in* q, int r)
{
    const int d = q->depth ? q->depth[r] : q->max_depth;
    return d < 0 ? 0 : d > q->max_depth ? q->max_depth : d;
}
/* The packet rule for list entry (r, t): -> red_size, 0 for a BAD packet; its source stream in *s, in *mask the carried generations (bit j - 1) and, from bit 4,
 * the number of generations that existed and were not carried */
static inline LC3RED_HD int32_t lc3red_packet(const lc3red_pack_in* q, int r, int t, int* s, int* mask)
{
    *mask = 0;
    if (r < 0 || r >= q->n_routes || t < 0 || t >= q->n_frames) return 0;
    const int c = lc3e_route(q->route_src, r, q->n_streams, q->counts, q->n_frames, s);
    if (c < 0 || t >= c) return 0;
    uintptr_t src = 0;
    const int32_t nb = lc3red_block(q, *s, t, &src);
    if (nb <= 0) return 0;
    const int d = lc3red_depth(q, r);
    int32_t acc = q->header_room + 1 + nb;                            /* header_room + max_frame_bytes + LC3RED_MAX_EXTRA fits an int32 (the calls' checks) */
    int m = 0, missed = 0;
    for (int j = 1; j <= d; j++) {
        const int32_t bs = lc3red_block(q, *s, t - j, &src);
        if (bs <= 0) continue;
        if (bs <= LC3RED_MAX_BLOCK && (long long)j * q->ts_step <= LC3RED_MAX_TS_OFFSET && (long long)acc + 4 + bs <= q->max_packet_bytes) { m |= 1 << (j - 1); acc += 4 + bs; }
        else missed++;
    }
    *mask = m | missed << 4;
    return acc;
}
static inline LC3RED_HD long long lc3red_advance(int32_t size, int align) { return size > 0 ? ((long long)size + align - 1) & ~(long long)(align - 1) : 0; }
/* a block's header (RFC 2198 section 3) as the 32-bit word whose little-endian bytes are the header: 1 | PT(7), timestamp offset (14), block length (10) */
static inline LC3RED_HD uint32_t lc3red_header(int pt, int ts_offset, int len)
{
    const uint32_t o = (uint32_t)ts_offset & 0x3FFFu, n = (uint32_t)len & 0x3FFu;
    return (0x80u | ((uint32_t)pt & 127u)) | (o >> 6) << 8 | ((o & 63u) << 2 | n >> 8) << 16 | (n & 255u) << 24;
}
/* The tail rule for entry g of stream s: -> its size and its source in *src, 0 for none */
static inline LC3RED_HD int32_t lc3red_tail(const lc3red_pack_in* q, int s, int g, uintptr_t* src)
{
    int s_ = 0;
    const int c = lc3e_route(NULL, s, q->n_streams, q->counts, q->n_frames, &s_);
    const int u = c - 1 - g;
    const int32_t nb = lc3red_block(q, s, u, src);
    return nb <= LC3RED_MAX_BLOCK ? nb : 0;
}

/* ---- the unpack rule ---- */
#if defined(__HIP_DEVICE_COMPILE__)
/* the four bytes at `at` as a big-endian word: one aligned word, two where `at` is not 4-aligned */
static inline __device__ uint32_t lc3red_fetch_be32(const uint8_t* ring, long long at)
{
    const uintptr_t a = (uintptr_t)ring + (uintptr_t)at;
    const uint32_t sh = (uint32_t)(a & 3);
    uint32_t v = lc3r_word(a);
    if (sh) v = __builtin_amdgcn_alignbyte(lc3r_word(a + 3), v, sh);
    return __builtin_amdgcn_perm(0, v, 0x00010203u);
}
#else
static inline uint32_t lc3red_fetch_be32(const uint8_t* ring, long long at)
{
    const uint8_t* p = ring + at;
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}
#endif
/* what an unpack call reads and writes (may be NULL: timestamp, block_pt, out_timestamp, out_gen, status) */
typedef struct {
    const int32_t* stream; const int32_t* seq; const long long* offsets; const int32_t* num_bytes; const int32_t* timestamp; const uint8_t* ring; const int32_t* block_pt;
    int32_t* out_stream; int32_t* out_seq; long long* out_offsets; int32_t* out_num_bytes; int32_t* out_timestamp; uint8_t* out_gen; uint8_t* status;
    long long ring_capacity;
    int32_t n_streams, max_red, ts_step;
} lc3red_unpack_io;
static inline LC3RED_HD void lc3red_slot_out(const lc3red_unpack_io* q, long long k, int32_t stream, int32_t seq, long long off, int32_t nb, int32_t ts, int gen)
{
    q->out_stream[k] = stream; q->out_seq[k] = seq; q->out_offsets[k] = off; q->out_num_bytes[k] = nb;
    if (q->out_timestamp) q->out_timestamp[k] = ts;
    if (q->out_gen) q->out_gen[k] = (uint8_t)gen;
}
/* The unpack rule for item i: fills its max_red + 1 slots and its status; -> the status.  drops[0 .. 2]: the blocks dropped for their type, their timestamp
 * offset and their length are added */
static inline LC3RED_HD int lc3red_unpack(const lc3red_unpack_io* q, long long i, int drops[3])
{
    const long long slot0 = i * (q->max_red + 1);
    const int s = q->stream[i];
    const long long off = q->offsets[i];
    const int32_t size = q->num_bytes[i];
    int st = LC3RED_OK, nf = 0, pos = 0;
    uint32_t hdr[LC3RED_MAX_DEPTH] = {0, 0, 0, 0}, b = 0;
    if (s < 0 || s >= q->n_streams) st = LC3RED_DROPPED;
    else if (off < 0 || size < 0 || off > q->ring_capacity - size) st = LC3RED_RANGE;                 /* ring_capacity >= 0 and size >= 0: no overflow */
    else {
        for (;;) {                                                    /* the header list: of a header behind the max_red-th only the first byte is read */
            if (pos >= size) { st = LC3RED_SHORT; break; }
            b = lc3r_fetch_byte(q->ring, off + pos);
            if (!(b & 128u)) break;
            if (pos + 4 > size) { st = LC3RED_SHORT; break; }
            if (nf < q->max_red) {
                const uint32_t w = lc3red_fetch_be32(q->ring, off + pos);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
                for (int k = 0; k < LC3RED_MAX_DEPTH; k++) if (k == nf) hdr[k] = w;
            }
            nf++; pos += 4;
        }
    }
    int sum = 0;
    if (st == LC3RED_OK) {
        pos += 1;
        if (nf > q->max_red) st = LC3RED_DEPTH;
        else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 0; k < LC3RED_MAX_DEPTH; k++) if (k < nf) sum += (int)(hdr[k] & 0x3FFu);
            if (pos + sum > size) st = LC3RED_LENGTH;
            else if (q->block_pt && q->block_pt[s] >= 0 && (uint32_t)q->block_pt[s] != (b & 127u)) st = LC3RED_PAYLOAD_TYPE;
        }
    }
    if (q->status) q->status[i] = (uint8_t)st;
    if (st != LC3RED_OK) {
        for (int k = 0; k <= q->max_red; k++) lc3red_slot_out(q, slot0 + k, -1, 0, 0, 0, 0, 0);
        return st;
    }
    const int32_t seq = q->seq[i], ts = q->timestamp ? q->timestamp[i] : 0;
    lc3red_slot_out(q, slot0, s, seq, off + pos + sum, size - pos - sum, ts, 0);
    long long at = off + pos;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < LC3RED_MAX_DEPTH; k++) {
        if (k >= q->max_red) break;
        const int len = (int)(hdr[k] & 0x3FFu), to = (int)(hdr[k] >> 10 & 0x3FFFu), pt = (int)(hdr[k] >> 24 & 127u);
        int why = -1;
        if (k >= nf) why = 3;                                         /* an unused slot */
        else if (q->block_pt && q->block_pt[s] >= 0 && q->block_pt[s] != pt) why = 0;
        else if (to == 0 || to % q->ts_step) why = 1;
        else if (len == 0) why = 2;
        if (why >= 0) {
            if (why < 3) drops[why]++;
            lc3red_slot_out(q, slot0 + 1 + k, -1, 0, 0, 0, 0, 0);
        } else {
            const int gen = to / q->ts_step;
            lc3red_slot_out(q, slot0 + 1 + k, s, (int32_t)(((uint32_t)seq - (uint32_t)gen) & 0xFFFFu), at, len, (int32_t)((uint32_t)ts - (uint32_t)to), gen > 255 ? 255 : gen);
        }
        if (k < nf) at += len;
    }
    return st;
}

/* one pack call: every pointer but the struct itself is a device pointer (those that may be NULL: see lc3red_pack_in; tail_bytes_out, tail_sizes_out, red_flags,
 * red_blocks, wire_total, route_stats) */
typedef struct {
    int32_t device, sync;
    long long max_packets;
    const long long* n_packets;
    lc3red_pack_in in;
    uint8_t* tail_bytes_out; int32_t* tail_sizes_out;
    void* wire;
    long long* red_offset; int32_t* red_size; uint8_t* red_flags; uint8_t* red_blocks; long long* wire_total; int32_t* route_stats;
    void* work; void* hip_stream;
} lc3red_pack_call;
/* one unpack call (may be NULL: see lc3red_unpack_io; stats) */
typedef struct {
    int32_t device, sync;
    long long n_items;
    lc3red_unpack_io io;
    int32_t* stats;
    void* hip_stream;
} lc3red_unpack_call;

#ifdef __cplusplus
extern "C" {
#endif
/* queue the kernels on q->hip_stream; wait for them only with q->sync.  0, or 1 where nothing was queued */
int lc3red_pack_run(const lc3red_pack_call* q);
int lc3red_unpack_run(const lc3red_unpack_call* q);
/* launches of a RED kernel by this process, by the kernel's symbol name in the code object; -1 for a name the library does not hold */
long long lc3red_launch_count(const char* kernel);
#ifdef __cplusplus
}
#endif
#endif
