/* lc3_rtp_shim.h -- RTP framing (include/lc3plus_batch.h "RTP framing": lc3plus_dec_batch_rtp_parse, lc3plus_{enc,dec}_batch_rtp_stamp, lc3plus_plan_rtp_parse,
 * lc3plus_plan_rtp_stamp): what the host C code (lc3_packet.c) and the sibling library that holds the RTP kernels (lc3_rtp.hip -> liblc3plus_rtp_hip.so) share.
 * The parse rule, the SSRC search, the stamp rule, the header's words and the per-route outputs are one text for the host functions and the kernels; they
 * differ only in how a datagram's bytes are fetched (lc3r_fetch12, lc3r_fetch_be16, lc3r_fetch_byte: plain bytes on the host, aligned 32-bit words realigned
 * in registers on the device).  The lc3rtp_* functions are the sibling's whole C ABI.  lc3_packet.c loads the sibling from its own directory on the first RTP
 * call; the code objects of the codec library, the probe library, the ingest library and the egress library hold none of this. */
#ifndef LC3_RTP_SHIM_H
#define LC3_RTP_SHIM_H
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC3R_HD __host__ __device__
#else
#define LC3R_HD
#endif

/* LC3PLUS_RTP_* of include/lc3plus_batch.h: an item's status (also the index of its word in stats), a packet's status, the marker modes */
enum { LC3R_OK = 0, LC3R_RANGE = 1, LC3R_SHORT = 2, LC3R_VERSION = 3, LC3R_RTCP = 4, LC3R_HEADER = 5, LC3R_PADDING = 6, LC3R_PAYLOAD_ROOM = 7, LC3R_UNKNOWN_SSRC = 8,
       LC3R_PAYLOAD_TYPE = 9, LC3R_STATUSES = 10, LC3R_STATS_WORDS = 16 };
enum { LC3R_STAMPED = 1, LC3R_ST_BAD_ROUTE = 2, LC3R_ST_OVERFLOW = 4, LC3R_ST_RANGE = 8 };
enum { LC3R_MARKER_NEVER = 0, LC3R_MARKER_AFTER_HOLE = 1 };
/* of the egress (lc3_egress_shim.h has the same values): a cell's SENT bit, a packet's overflow flag, the stride of a route's stats and its count's word */
enum { LC3R_EGR_SENT = 1, LC3R_EGR_PKT_OVERFLOW = 1, LC3R_EGR_STATS_WORDS = 4, LC3R_EGR_ST_COUNT = 0 };
enum { LC3R_FIXED = 12, LC3R_MAX_PAYLOAD_ROOM = 4096 };
#define LC3R_MAX_ITEMS (1LL << 29)
/* The SSRC table is staged in LDS up to this many entries (key and stream: 8 bytes each, 32 KiB), a fifth of a CU's 160 KiB and half of what one workgroup
 * may have.  The parse kernel's workgroups are 1 024 lanes, one per CU, so that a CU stages the table once.  Above the budget every lane searches the table where
 * it lies, in global memory. */
enum { LC3R_THREADS = 256, LC3R_PARSE_THREADS = 1024, LC3R_LDS_ENTRIES = 4096 };

/* ---- a datagram's bytes ---- */
#if defined(__HIP_DEVICE_COMPILE__)
/* the aligned 32-bit word that holds the byte at address a */
static inline __device__ uint32_t lc3r_word(uintptr_t a) { return *(const uint32_t*)(a & ~(uintptr_t)3); }
/* the twelve bytes at `at` as three big-endian words: three aligned words, a fourth where `at` is not 4-aligned (it then holds byte 11), realigned with
 * v_alignbyte_b32 and turned with v_perm_b32 */
static inline __device__ void lc3r_fetch12(const uint8_t* ring, long long at, uint32_t w[3])
{
    const uintptr_t a = (uintptr_t)ring + (uintptr_t)at;
    const uint32_t sh = (uint32_t)(a & 3);
    uint32_t v0 = lc3r_word(a), v1 = lc3r_word(a + 4), v2 = lc3r_word(a + 8);
    if (sh) {
        const uint32_t v3 = lc3r_word(a + 12);
        v0 = __builtin_amdgcn_alignbyte(v1, v0, sh); v1 = __builtin_amdgcn_alignbyte(v2, v1, sh); v2 = __builtin_amdgcn_alignbyte(v3, v2, sh);
    }
    w[0] = __builtin_amdgcn_perm(0, v0, 0x00010203u); w[1] = __builtin_amdgcn_perm(0, v1, 0x00010203u); w[2] = __builtin_amdgcn_perm(0, v2, 0x00010203u);
}
static inline __device__ uint32_t lc3r_fetch_byte(const uint8_t* ring, long long at)
{
    const uintptr_t a = (uintptr_t)ring + (uintptr_t)at;
    return (lc3r_word(a) >> ((a & 3) * 8)) & 255u;
}
/* the big-endian 16-bit value at `at`: one aligned word, two where its bytes lie on both sides of a word boundary */
static inline __device__ uint32_t lc3r_fetch_be16(const uint8_t* ring, long long at)
{
    const uintptr_t a = (uintptr_t)ring + (uintptr_t)at;
    const uint32_t sh = (uint32_t)(a & 3);
    uint32_t v = lc3r_word(a);
    if (sh == 3) v = __builtin_amdgcn_alignbyte(lc3r_word(a + 1), v, 3); else v >>= sh * 8;
    return __builtin_amdgcn_perm(0, v, 0x0c0c0001u);                 /* byte 0 of v above byte 1, zeroes above them */
}
#else
static inline void lc3r_fetch12(const uint8_t* ring, long long at, uint32_t w[3])
{
    const uint8_t* p = ring + at;
    for (int k = 0; k < 3; k++) w[k] = (uint32_t)p[4 * k] << 24 | (uint32_t)p[4 * k + 1] << 16 | (uint32_t)p[4 * k + 2] << 8 | p[4 * k + 3];
}
static inline uint32_t lc3r_fetch_byte(const uint8_t* ring, long long at) { return ring[at]; }
static inline uint32_t lc3r_fetch_be16(const uint8_t* ring, long long at) { return (uint32_t)ring[at] << 8 | ring[at + 1]; }
#endif

/* ---- the parse rule ---- */
/* The SSRC search: the lower bound of ssrc in key[0 .. n) compared as uint32, then the entry's stream.  -> the stream, or -1 where no equal key stands there
 * or its stream lies outside [0, n_streams).  Whatever order the table is in, host and device walk it alike */
static inline LC3R_HD int lc3r_lookup(const int32_t* key, const int32_t* strm, int n, uint32_t ssrc, int n_streams)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)key[mid] < ssrc) lo = mid + 1; else hi = mid;
    }
    if (lo >= n || (uint32_t)key[lo] != ssrc) return -1;
    const int s = strm[lo];
    return s < 0 || s >= n_streams ? -1 : s;
}
/* what an item becomes */
typedef struct { int32_t stream, seq, num_bytes, timestamp; long long offset; uint8_t marker, status; } lc3r_item;
/* The parse rule for one datagram ring[off .. off + size): the first check that fails is the status.  key / strm: the SSRC table, wherever it lies */
static inline LC3R_HD lc3r_item lc3r_parse(const uint8_t* ring, long long capacity, long long off, int32_t size, const int32_t* key, const int32_t* strm, int n_ssrc,
                                           int n_streams, const int32_t* payload_type, int payload_room)
{
    lc3r_item it = {-1, 0, 0, 0, 0, 0, LC3R_OK};
    if (off < 0 || size < 0 || off > capacity - size) { it.status = LC3R_RANGE; return it; }          /* capacity >= 0 and size >= 0: no overflow */
    if (size < LC3R_FIXED) { it.status = LC3R_SHORT; return it; }
    uint32_t w[3];
    lc3r_fetch12(ring, off, w);
    const uint32_t b0 = w[0] >> 24, b1 = (w[0] >> 16) & 255u;
    if (b0 >> 6 != 2) { it.status = LC3R_VERSION; return it; }
    if (b1 >= 192 && b1 <= 223) { it.status = LC3R_RTCP; return it; }
    int h = LC3R_FIXED + 4 * (int)(b0 & 15u);
    if (h > size) { it.status = LC3R_HEADER; return it; }
    if (b0 & 16u) {
        if (h + 4 > size) { it.status = LC3R_HEADER; return it; }
        h += 4 + 4 * (int)lc3r_fetch_be16(ring, off + h + 2);
        if (h > size) { it.status = LC3R_HEADER; return it; }
    }
    int pad = 0;
    if (b0 & 32u) {
        pad = (int)lc3r_fetch_byte(ring, off + size - 1);
        if (pad == 0 || h + pad > size) { it.status = LC3R_PADDING; return it; }
    }
    const int left = size - h - pad;
    if (left < payload_room) { it.status = LC3R_PAYLOAD_ROOM; return it; }
    const int s = lc3r_lookup(key, strm, n_ssrc, w[2], n_streams);
    if (s < 0) { it.status = LC3R_UNKNOWN_SSRC; return it; }
    if (payload_type && payload_type[s] >= 0 && (uint32_t)payload_type[s] != (b1 & 127u)) { it.status = LC3R_PAYLOAD_TYPE; return it; }
    it.stream = s; it.seq = (int32_t)(w[0] & 0xFFFFu); it.offset = off + h + payload_room; it.num_bytes = left - payload_room; it.timestamp = (int32_t)w[1];
    it.marker = (uint8_t)(b1 >> 7);
    return it;
}
/* the item arrays of a parse call (timestamp, marker, status: each may be NULL) */
typedef struct { int32_t* stream; int32_t* seq; long long* offsets; int32_t* num_bytes; int32_t* timestamp; uint8_t* marker; uint8_t* status; } lc3r_items;
static inline LC3R_HD void lc3r_item_out(const lc3r_items* o, long long i, const lc3r_item* it)
{
    o->stream[i] = it->stream; o->seq[i] = it->seq; o->offsets[i] = it->offset; o->num_bytes[i] = it->num_bytes;
    if (o->timestamp) o->timestamp[i] = it->timestamp;
    if (o->marker) o->marker[i] = it->marker;
    if (o->status) o->status[i] = it->status;
}

/* ---- the stamp rule ---- */
/* the packet list and the per-route tables a stamp call reads (pkt_flags, cell_status, resume, route_stats: each may be NULL) */
typedef struct {
    const int32_t* route; const int32_t* seq; const int32_t* frame; const long long* offset; const int32_t* size; const uint8_t* flags;
    const int32_t* ssrc; const int32_t* ts_base; const int32_t* payload_type; const uint8_t* cell_status; const uint8_t* resume; const int32_t* route_stats;
    int32_t n_routes, n_frames, ts_step, marker_mode, header_room, payload_room;
    long long wire_capacity;
} lc3r_stamp_in;
/* The stamp rule for packet p: -> its status; where that is STAMPED, the header's three words in hdr (hdr[k] holds bytes 4k .. 4k + 3 of the header, byte
 * 4k lowest: stored as little-endian words they are the header) and the header's offset in the wire buffer in *at */
static inline LC3R_HD int lc3r_stamp(const lc3r_stamp_in* q, long long p, uint32_t hdr[3], long long* at)
{
    const int r = q->route[p];
    if (r < 0 || r >= q->n_routes) return LC3R_ST_BAD_ROUTE;
    if (q->flags && (q->flags[p] & LC3R_EGR_PKT_OVERFLOW)) return LC3R_ST_OVERFLOW;
    const long long off = q->offset[p];
    const int32_t size = q->size[p];
    const int t = q->frame[p];
    if (off < 0 || size < q->header_room || off > q->wire_capacity - size || t < 0 || t >= q->n_frames) return LC3R_ST_RANGE;     /* size >= 12: no overflow */
    uint32_t m = 0;
    if (q->marker_mode == LC3R_MARKER_AFTER_HOLE)
        m = t > 0 ? !(q->cell_status[(size_t)r * q->n_frames + t - 1] & LC3R_EGR_SENT) : q->resume ? q->resume[r] != 0 : 0;
    const uint32_t seq = (uint32_t)q->seq[p] & 0xFFFFu, ts = (uint32_t)q->ts_base[r] + (uint32_t)t * (uint32_t)q->ts_step, ssrc = (uint32_t)q->ssrc[r];
    hdr[0] = 0x80u | (m << 7 | ((uint32_t)q->payload_type[r] & 127u)) << 8 | (seq >> 8) << 16 | (seq & 255u) << 24;
    hdr[1] = ts >> 24 | (ts >> 16 & 255u) << 8 | (ts >> 8 & 255u) << 16 | (ts & 255u) << 24;
    hdr[2] = ssrc >> 24 | (ssrc >> 16 & 255u) << 8 | (ssrc >> 8 & 255u) << 16 | (ssrc & 255u) << 24;
    *at = off + q->header_room - q->payload_room - LC3R_FIXED;
    return LC3R_STAMPED;
}
/* the header's twelve bytes into the wire buffer: three word stores where the address is 4-aligned, twelve byte stores otherwise */
static inline LC3R_HD void lc3r_header_out(uint8_t* wire, long long at, const uint32_t hdr[3])
{
    uint8_t* d = wire + at;
#if defined(__HIP_DEVICE_COMPILE__)
    if (!((uintptr_t)d & 3)) { uint32_t* d4 = (uint32_t*)d; d4[0] = hdr[0]; d4[1] = hdr[1]; d4[2] = hdr[2]; return; }
#endif
    for (int k = 0; k < LC3R_FIXED; k++) d[k] = (uint8_t)(hdr[k >> 2] >> ((k & 3) * 8));
}
/* a route's outputs: next_ts and next_resume from its count c = the egress's stats word clamped to the call, n_frames without route_stats */
static inline LC3R_HD void lc3r_route_out(const lc3r_stamp_in* q, int r, int32_t* next_ts, uint8_t* next_resume)
{
    int c = q->n_frames;
    if (q->route_stats) { c = q->route_stats[(size_t)r * LC3R_EGR_STATS_WORDS + LC3R_EGR_ST_COUNT]; c = c < 0 ? 0 : c > q->n_frames ? q->n_frames : c; }
    if (next_ts) next_ts[r] = (int32_t)((uint32_t)q->ts_base[r] + (uint32_t)c * (uint32_t)q->ts_step);
    if (next_resume)
        next_resume[r] = c == 0 ? (q->resume ? q->resume[r] : 0) : (uint8_t)!(q->cell_status[(size_t)r * q->n_frames + c - 1] & LC3R_EGR_SENT);
}

/* one parse call: every pointer but the struct itself is a device pointer (those that may be NULL: payload_type, out.timestamp, out.marker, out.status, stats) */
typedef struct {
    int32_t device, n_streams, n_ssrc, payload_room, sync;
    long long n_items, ring_capacity;
    const void* ring; const long long* dg_offsets; const int32_t* dg_sizes; const int32_t* ssrc_key; const int32_t* ssrc_stream; const int32_t* payload_type;
    lc3r_items out; int32_t* stats;
    void* hip_stream;
} lc3rtp_parse_call;
/* one stamp call (may be NULL: in.flags, in.cell_status, in.resume, in.route_stats, pkt_status, next_ts, next_resume) */
typedef struct {
    int32_t device, sync;
    long long max_packets;
    const long long* n_packets;
    lc3r_stamp_in in;
    void* wire; uint8_t* pkt_status; int32_t* next_ts; uint8_t* next_resume;
    void* hip_stream;
} lc3rtp_stamp_call;

#ifdef __cplusplus
extern "C" {
#endif
/* queue the kernels on q->hip_stream; wait for them only with q->sync.  0, or 1 where nothing was queued */
int lc3rtp_parse_run(const lc3rtp_parse_call* q);
int lc3rtp_stamp_run(const lc3rtp_stamp_call* q);
/* launches of an RTP kernel by this process, by the kernel's symbol name in the code object; -1 for a name the library does not hold */
long long lc3rtp_launch_count(const char* kernel);
#ifdef __cplusplus
}
#endif
#endif
