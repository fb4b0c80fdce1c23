/* lc3_fec_shim.h -- generic forward error correction, RFC 5109 (include/lc3plus_batch.h "Generic FEC": lc3plus_{enc,dec}_batch_fec_encode,
 * lc3plus_dec_batch_fec_recover, lc3plus_plan_fec_encode, lc3plus_plan_fec_recover): what the host C code (lc3_packet.c) and the sibling library that holds the FEC
 * kernels (lc3_fec.hip -> liblc3plus_fec_hip.so) share.  The group rule, the member rule, the fold of a group's header fields, the FEC header's bytes, the state
 * handed to the next call, the lookup and the verdict of the recovery are one text for the host functions and the kernels; they differ only in how payload bytes
 * are fetched and XORed (plain bytes on the host, aligned 32-bit words realigned in registers on the device, the idiom of lc3_rtp_shim.h).  The copy layout is
 * the egress's (lc3_egress_shim.h), by inclusion.  The lc3fec_* functions are the sibling's whole C ABI.  lc3_packet.c loads the sibling from its own directory on
 * the first FEC call; the code objects of the other libraries hold none of this. */
#ifndef LC3_FEC_SHIM_H
#define LC3_FEC_SHIM_H
#include <stdint.h>
#include <stddef.h>
#include "lc3_egress_shim.h"
#include "lc3_rtp_shim.h"

#define LC3FEC_HD LC3E_HD

/* LC3PLUS_FEC_* of include/lc3plus_batch.h */
enum { LC3FEC_MAX_GROUP = 16, LC3FEC_STATE_WORDS = 8, LC3FEC_PKT_EMPTY = 2, LC3FEC_HEADER = 14, LC3FEC_HEADER_LONG = 18, LC3FEC_MAX_LEN = 65535,
       LC3FEC_MAX_PKT = 1 << 20, LC3FEC_MAX_BITS = 48 };
enum { LC3FEC_S_FILL = 0, LC3FEC_S_K = 1, LC3FEC_S_SN = 2, LC3FEC_S_MASK = 3, LC3FEC_S_HDR = 4, LC3FEC_S_TS = 5, LC3FEC_S_LEN = 6, LC3FEC_S_MAX = 7 };
enum { LC3FEC_RS_WORDS = 4, LC3FEC_RS_GROUPS = 0, LC3FEC_RS_PACKETS = 1, LC3FEC_RS_MEDIA = 2, LC3FEC_RS_BYTES = 3 };
enum { LC3FEC_RECOVERED = 0, LC3FEC_DROPPED = 1, LC3FEC_RANGE = 2, LC3FEC_SHORT = 3, LC3FEC_BAD_HEADER = 4, LC3FEC_LENGTH = 5, LC3FEC_COMPLETE = 6, LC3FEC_MISSING = 7,
       LC3FEC_PARTIAL = 8, LC3FEC_OVERFLOW = 9, LC3FEC_STATUSES = 10, LC3FEC_STATS_WORDS = 16 };
/* the scan over the routes runs in tiles of LC3FEC_TILE: LC3FEC_THREADS lanes with LC3FEC_ITEMS neighbouring routes each; LC3FEC_ENC_LANES lanes own a group of
 * the encoder, LC3FEC_REC_LANES (a wave) a recovering item */
enum { LC3FEC_THREADS = 256, LC3FEC_ITEMS = 4, LC3FEC_TILE = LC3FEC_THREADS * LC3FEC_ITEMS, LC3FEC_ENC_LANES = 8, LC3FEC_REC_LANES = 64 };
#define LC3FEC_NO_ENTRY 0x7FFFFFFF
#define LC3FEC_MAX_PACKETS 0x7FFFFFFFLL
#define LC3FEC_MAX_STRIDE (1LL << 30)

/* The workspace of an encode call, in this order: map [n_routes][n_frames] int32, the lowest list entry that names the cell or LC3FEC_NO_ENTRY; the tiles' sums
 * and then bases [n_tiles] int64; qbase [n_routes] int64, the index of each route's first FEC entry; fseq [n_routes] int32, each route's fec_seq_base as the call
 * found it (next_fec_seq may be the same array: it is written by the lane that has made this copy, and the records are numbered from the copy) */
static inline LC3FEC_HD long long lc3fec_tiles(long long n_routes) { return (n_routes + LC3FEC_TILE - 1) / LC3FEC_TILE; }
static inline LC3FEC_HD long long lc3fec_work_sums(long long n_routes, long long n_frames) { return (4 * n_routes * n_frames + 7) & ~7LL; }
static inline LC3FEC_HD long long lc3fec_work_qbase(long long n_routes, long long n_frames) { return lc3fec_work_sums(n_routes, n_frames) + 8 * lc3fec_tiles(n_routes); }
static inline LC3FEC_HD long long lc3fec_work_fseq(long long n_routes, long long n_frames) { return lc3fec_work_qbase(n_routes, n_frames) + 8 * n_routes; }
static inline LC3FEC_HD long long lc3fec_work_bytes(long long n_routes, long long n_frames) { return lc3fec_work_fseq(n_routes, n_frames) + ((4 * n_routes + 7) & ~7LL); }
/* the workspace of a recover call: table [n_streams][window] int32 */
static inline LC3FEC_HD long long lc3fec_recover_work_bytes(long long n_streams, long long window) { return 4 * n_streams * window; }

/* big-endian fields of a packet */
#if defined(__HIP_DEVICE_COMPILE__)
/* the four bytes at `at` as a big-endian word: one aligned word, two where `at` is not 4-aligned */
static inline __device__ uint32_t lc3fec_fetch_be32(const uint8_t* ring, long long at)
{
    const uintptr_t a = (uintptr_t)ring + (uintptr_t)at;
    const uint32_t sh = (uint32_t)(a & 3);
    uint32_t v = lc3r_word(a);
    if (sh) v = __builtin_amdgcn_alignbyte(lc3r_word(a + 3), v, sh);
    return __builtin_amdgcn_perm(0, v, 0x00010203u);
}
#else
static inline uint32_t lc3fec_fetch_be32(const uint8_t* ring, long long at)
{
    const uint8_t* p = ring + at;
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
}
#endif

/* ---- the encoder ---- */
/* what an encode call reads (may be NULL: pkt_status, route_stats, flush, state_in with acc_in) */
typedef struct {
    const long long* n_packets; const int32_t* pkt_route; const int32_t* pkt_frame; const long long* pkt_offset; const int32_t* pkt_size; const uint8_t* pkt_status;
    const uint8_t* wire; const int32_t* seq_base; const int32_t* route_stats; const int32_t* group; const uint8_t* flush; const int32_t* fec_seq_base;
    const int32_t* state_in; const uint8_t* acc_in;
    long long max_packets, wire_capacity, max_fec_packets, fec_capacity, fec_stride;
    int32_t header_room, payload_room, n_routes, n_frames, acc_stride, fec_header_room, carry;  /* carry: state_out and acc_out are given */
} lc3fec_enc_in;
/* what it writes (may be NULL: fec_flags, fec_mask, next_fec_seq, route_stats_out, state_out with acc_out) */
typedef struct {
    long long* n_fec; int32_t* fec_route; int32_t* fec_seq; int32_t* fec_frame; long long* fec_offset; int32_t* fec_size; uint8_t* fec_flags; int32_t* fec_mask;
    int32_t* next_fec_seq; int32_t* route_stats_out; int32_t* state_out; uint8_t* acc_out; uint8_t* fec_wire;
} lc3fec_enc_out;

static inline LC3FEC_HD long long lc3fec_count(const long long* n_packets, long long max_packets)
{
    const long long n = *n_packets;
    return n < 0 ? 0 : n > max_packets ? max_packets : n;
}
/* a route's count c: the egress's stats word clamped to the call, n_frames without route_stats (the stamp's reading) */
static inline LC3FEC_HD int lc3fec_route_count(const lc3fec_enc_in* q, int r)
{
    if (!q->route_stats) return q->n_frames;
    const int c = q->route_stats[(size_t)r * LC3E_STATS_WORDS + LC3E_ST_COUNT];
    return c < 0 ? 0 : c > q->n_frames ? q->n_frames : c;
}
/* The member rule for list entry p: -> its cell r * n_frames + t, or -1 where it is no member */
static inline LC3FEC_HD long long lc3fec_entry_cell(const lc3fec_enc_in* q, long long p)
{
    const int r = q->pkt_route[p], t = q->pkt_frame[p];
    if (r < 0 || r >= q->n_routes || t < 0 || t >= lc3fec_route_count(q, r)) return -1;
    if (q->pkt_status && !(q->pkt_status[p] & LC3R_STAMPED)) return -1;
    const long long off = q->pkt_offset[p];
    const int32_t size = q->pkt_size[p];
    if (off < 0 || size < q->header_room || size > LC3FEC_MAX_PKT || off > q->wire_capacity - size) return -1;       /* the protect call's RANGE */
    if (size - q->header_room + q->payload_room > LC3FEC_MAX_LEN) return -1;
    return (long long)r * q->n_frames + t;
}
/* the member at cell (r, t): -> 1, the offset of byte 12 of its RTP packet in *at and its length (the packet's bytes less 12) in *len; 0 for a hole */
static inline LC3FEC_HD int lc3fec_member(const lc3fec_enc_in* q, const int32_t* map, int r, int t, long long* at, int32_t* len)
{
    const int32_t p = map[(size_t)r * q->n_frames + t];
    if (p == LC3FEC_NO_ENTRY) return 0;
    *at = q->pkt_offset[p] + q->header_room - q->payload_room;
    *len = q->pkt_size[p] - q->header_room + q->payload_room;
    return 1;
}

/* The group rule of a route: c its count, F and K the carried group's fill and size (0 0: none), k the size of the groups that open in this call, a the
 * positions that go to the carried group, ng the groups the call touches, open whether the last of them stays open, nclosed = ng - open */
typedef struct { int c, F, K, k, a, ng, nclosed, open; } lc3fec_plan;
static inline LC3FEC_HD lc3fec_plan lc3fec_route_plan(const lc3fec_enc_in* q, int r)
{
    lc3fec_plan p;
    p.c = lc3fec_route_count(q, r);
    const int k = q->group[r];
    p.k = k < 0 ? 0 : k > LC3FEC_MAX_GROUP ? LC3FEC_MAX_GROUP : k;
    p.F = p.K = 0;
    if (q->state_in) {
        const int32_t* st = q->state_in + (size_t)r * LC3FEC_STATE_WORDS;
        p.F = st[LC3FEC_S_FILL]; p.K = st[LC3FEC_S_K];
        if (p.K < 1 || p.K > LC3FEC_MAX_GROUP || p.F < 1 || p.F >= p.K) p.F = p.K = 0;    /* a state that no call has written holds no group */
    }
    p.a = p.F ? (p.K - p.F < p.c ? p.K - p.F : p.c) : 0;
    const int rest = p.c - p.a, fresh = p.k ? (rest + p.k - 1) / p.k : 0;
    p.ng = (p.a > 0) + fresh;
    p.open = 0;
    if (p.ng) {
        const int full = fresh ? rest - (fresh - 1) * p.k == p.k : p.F + p.a == p.K;
        p.open = !(full || (q->flush && q->flush[r]));
    }
    p.nclosed = p.ng - p.open;
    return p;
}
/* group g < ng of a plan: its positions [t0, t1) of this call, its size K, the positions F0 it had passed before the call, whether it closes */
typedef struct { int t0, t1, K, F0, closes; } lc3fec_group;
static inline LC3FEC_HD lc3fec_group lc3fec_group_of(const lc3fec_plan* p, int g)
{
    lc3fec_group G;
    if (p->a > 0 && g == 0) { G.t0 = 0; G.t1 = p->a; G.K = p->K; G.F0 = p->F; }
    else {
        G.t0 = p->a + (g - (p->a > 0)) * p->k;
        G.t1 = G.t0 + p->k < p->c ? G.t0 + p->k : p->c;
        G.K = p->k; G.F0 = 0;
    }
    G.closes = g < p->nclosed;
    return G;
}

/* A group's fields: the mask as it stands on the wire (position i is bit 15 - i), the XOR of the members' bytes 0 (its low 6 bits) and 1 (hdr = b0 | b1 << 8),
 * timestamps and lengths, the largest length; dead: the group was dropped for acc_stride and protects nothing; sn: its SN base */
typedef struct { uint32_t mask, hdr, ts, len, sn; int32_t plen, carried, dead, members; } lc3fec_fold;
/* The fold of group G of route r over the members at[i], len[i] (len < 0: a hole) of its positions t0 + i, behind what the state carries */
static inline LC3FEC_HD lc3fec_fold lc3fec_fold_group(const lc3fec_enc_in* q, int r, const lc3fec_group* G, const long long* at, const int32_t* len)
{
    lc3fec_fold f;
    f.mask = f.hdr = f.ts = f.len = 0; f.plen = 0; f.carried = 0; f.dead = 0; f.members = 0;
    f.sn = ((uint32_t)q->seq_base[r] + (uint32_t)G->t0) & 0xFFFFu;
    if (G->F0 > 0) {
        const int32_t* st = q->state_in + (size_t)r * LC3FEC_STATE_WORDS;
        f.sn = (uint32_t)st[LC3FEC_S_SN] & 0xFFFFu;
        f.mask = (uint32_t)st[LC3FEC_S_MASK] & 0xFFFFu & ~(0xFFFFu >> G->F0);
        f.hdr = (uint32_t)st[LC3FEC_S_HDR] & 0xFF3Fu; f.ts = (uint32_t)st[LC3FEC_S_TS]; f.len = (uint32_t)st[LC3FEC_S_LEN] & 0xFFFFu;
        f.plen = st[LC3FEC_S_MAX];
        if (f.plen < 0 || f.plen > q->acc_stride || f.plen > LC3FEC_MAX_LEN) { f.dead = 1; f.plen = 0; }
        f.carried = f.plen;
    }
    for (int i = 0; i < G->t1 - G->t0; i++) {
        if (len[i] < 0 || f.dead) continue;
        const uint32_t b0 = lc3r_fetch_byte(q->wire, at[i] - 12), b1 = lc3r_fetch_byte(q->wire, at[i] - 11);
        f.mask |= 0x8000u >> (G->F0 + i);
        f.hdr ^= (b0 & 0x3Fu) | b1 << 8;
        f.ts ^= lc3fec_fetch_be32(q->wire, at[i] - 8);
        f.len ^= (uint32_t)len[i];
        if (len[i] > f.plen) f.plen = len[i];
        f.members++;
    }
    if (f.dead) { f.mask = f.hdr = f.ts = f.len = 0; f.plen = 0; f.carried = 0; }
    return f;
}
/* the FEC header and the level-0 header as four words whose little-endian bytes are the fourteen bytes (RFC 5109 7.3, 7.4 with E = 0 and L = 0) */
static inline LC3FEC_HD void lc3fec_header(const lc3fec_fold* f, uint32_t w[4])
{
    const uint32_t pl = (uint32_t)f->plen;
    w[0] = (f->hdr & 0x3Fu) | (f->hdr >> 8 & 255u) << 8 | (f->sn >> 8) << 16 | (f->sn & 255u) << 24;
    w[1] = f->ts >> 24 | (f->ts >> 16 & 255u) << 8 | (f->ts >> 8 & 255u) << 16 | (f->ts & 255u) << 24;
    w[2] = (f->len >> 8 & 255u) | (f->len & 255u) << 8 | (pl >> 8 & 255u) << 16 | (pl & 255u) << 24;
    w[3] = (f->mask >> 8 & 255u) | (f->mask & 255u) << 8;
}
static inline LC3FEC_HD void lc3fec_header_out(uint8_t* d, const uint32_t w[4])
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < LC3FEC_HEADER; k++) d[k] = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));
}
/* The record of closed group gi (its index among the route's groups of this call) at entry e of the list, seq0 the route's fec_seq_base (the workspace's copy).
 * -> 1 where the packet's bytes are to be written */
static inline LC3FEC_HD int lc3fec_emit(const lc3fec_enc_in* q, const lc3fec_enc_out* o, int r, int gi, const lc3fec_group* G, const lc3fec_fold* f, long long e,
                                        int32_t seq0, int32_t* size_out)
{
    const int32_t size = f->mask ? q->fec_header_room + LC3FEC_HEADER + f->plen : 0;
    const long long off = e * q->fec_stride;
    int flags = 0;
    if (!f->mask) flags = LC3FEC_PKT_EMPTY;
    else if (e >= q->max_fec_packets || size > q->fec_stride || off > q->fec_capacity - size) flags = LC3E_PKT_OVERFLOW;
    *size_out = size;
    if (e < q->max_fec_packets) {
        o->fec_route[e] = r; o->fec_seq[e] = (int32_t)((uint32_t)seq0 + (uint32_t)gi); o->fec_frame[e] = G->t1 - 1; o->fec_offset[e] = off;
        o->fec_size[e] = size;
        if (o->fec_flags) o->fec_flags[e] = (uint8_t)flags;
        if (o->fec_mask) o->fec_mask[e] = (int32_t)f->mask;
    }
    return !flags;
}
/* The state an open group hands on.  -> 1 where its XOR goes to the accumulator, 0 where the group is dropped (or was) and the accumulator is zeroed */
static inline LC3FEC_HD int lc3fec_state_out(const lc3fec_enc_in* q, int32_t* st, const lc3fec_group* G, const lc3fec_fold* f)
{
    const int drop = f->dead || f->plen > q->acc_stride;
    st[LC3FEC_S_FILL] = G->F0 + G->t1 - G->t0; st[LC3FEC_S_K] = G->K; st[LC3FEC_S_SN] = (int32_t)f->sn;
    st[LC3FEC_S_MASK] = drop ? 0 : (int32_t)f->mask; st[LC3FEC_S_HDR] = drop ? 0 : (int32_t)f->hdr; st[LC3FEC_S_TS] = drop ? 0 : (int32_t)f->ts;
    st[LC3FEC_S_LEN] = drop ? 0 : (int32_t)f->len; st[LC3FEC_S_MAX] = drop ? -1 : f->plen;
    return !drop;
}

/* ---- the recovery ---- */
/* what a recover call reads and writes (may be NULL: status, stats) */
typedef struct {
    uint8_t* ring; const long long* dg_offsets; const int32_t* dg_sizes; const int32_t* stream; const int32_t* seq;
    const int32_t* fec_stream; const long long* fec_offsets; const int32_t* fec_num_bytes; const int32_t* ssrc;
    long long* rec_dg_offsets; int32_t* rec_dg_sizes; int32_t* rec_seq; uint8_t* status;
    long long ring_capacity, n_items, n_fec, rec_offset, rec_stride;
    int32_t n_streams, window;
} lc3fec_rec_io;
/* The lookup: the packet of stream s with sequence number sn.  -> 1, the offset of its byte 12 in *at and its length in *len; 0 where it is missing */
static inline LC3FEC_HD int lc3fec_lookup(const lc3fec_rec_io* q, const int32_t* table, int s, uint32_t sn, long long* at, int32_t* len)
{
    const int32_t i = table[(size_t)s * q->window + (sn & (uint32_t)(q->window - 1))];
    if (i == LC3FEC_NO_ENTRY) return 0;
    if (q->stream[i] != s || ((uint32_t)q->seq[i] & 0xFFFFu) != sn) return 0;
    const long long off = q->dg_offsets[i];
    const int32_t size = q->dg_sizes[i];
    if (off < 0 || size < LC3R_FIXED || off > q->ring_capacity - size) return 0;
    *at = off + LC3R_FIXED; *len = size - LC3R_FIXED;
    return 1;
}
/* an FEC item's header: L its mask's width (0: 16 bits, 1: 48), mask with position i at bit 47 - i, hl the bytes in front of the level-0 payload */
typedef struct { uint32_t b0, b1, sn, ts, len, plen; unsigned long long mask; int hl; } lc3fec_item;
/* The checks 1 ... 5 of item f: -> 0 and the header in *h, or the status */
static inline LC3FEC_HD int lc3fec_item_header(const lc3fec_rec_io* q, long long f, lc3fec_item* h)
{
    const int s = q->fec_stream[f];
    const long long off = q->fec_offsets[f];
    const int32_t size = q->fec_num_bytes[f];
    if (s < 0 || s >= q->n_streams) return LC3FEC_DROPPED;
    if (off < 0 || size < 0 || off > q->ring_capacity - size) return LC3FEC_RANGE;
    if (size < LC3FEC_HEADER) return LC3FEC_SHORT;
    uint32_t w[3];
    lc3r_fetch12(q->ring, off, w);
    h->b0 = w[0] >> 24; h->b1 = w[0] >> 16 & 255u; h->sn = w[0] & 0xFFFFu; h->ts = w[1]; h->len = w[2] >> 16; h->plen = w[2] & 0xFFFFu;
    const int L = h->b0 >> 6 & 1;
    h->hl = L ? LC3FEC_HEADER_LONG : LC3FEC_HEADER;
    if (size < h->hl) return LC3FEC_SHORT;
    h->mask = (unsigned long long)lc3r_fetch_be16(q->ring, off + 12) << 32;
    if (L) h->mask |= lc3fec_fetch_be32(q->ring, off + 14);
    if ((h->b0 & 128u) || !h->mask || !h->plen) return LC3FEC_BAD_HEADER;
    if (h->hl + (int32_t)h->plen > size) return LC3FEC_LENGTH;
    return 0;
}
/* The verdict of item f: its status, its three outputs, and for a RECOVERED item the twelve header bytes of its slot */
static inline LC3FEC_HD int lc3fec_verdict(const lc3fec_rec_io* q, const int32_t* table, long long f)
{
    lc3fec_item h;
    int st = lc3fec_item_header(q, f, &h);
    uint32_t hdr = 0, ts = 0, len = 0, miss_sn = 0;
    if (!st) {
        const int s = q->fec_stream[f];
        int missing = 0;
        for (int i = 0; i < LC3FEC_MAX_BITS; i++) {
            if (!(h.mask >> (LC3FEC_MAX_BITS - 1 - i) & 1)) continue;
            const uint32_t sn = (h.sn + (uint32_t)i) & 0xFFFFu;
            long long at = 0;
            int32_t n = 0;
            if (!lc3fec_lookup(q, table, s, sn, &at, &n)) { missing++; miss_sn = sn; continue; }
            hdr ^= (lc3r_fetch_byte(q->ring, at - 12) & 0x3Fu) | lc3r_fetch_byte(q->ring, at - 11) << 8;
            ts ^= lc3fec_fetch_be32(q->ring, at - 8);
            len ^= (uint32_t)n & 0xFFFFu;
        }
        const uint32_t rl = h.len ^ len;
        const long long slot = q->rec_offset + f * q->rec_stride;
        if (missing == 0) st = LC3FEC_COMPLETE;
        else if (missing > 1) st = LC3FEC_MISSING;
        else if (rl > h.plen) st = LC3FEC_PARTIAL;
        else if (LC3R_FIXED + (long long)rl > q->rec_stride || slot > q->ring_capacity - q->rec_stride) st = LC3FEC_OVERFLOW;
        else {
            const uint32_t b0 = 0x80u | ((h.b0 ^ hdr) & 0x3Fu), b1 = (h.b1 ^ (hdr >> 8)) & 255u, t = h.ts ^ ts, ss = (uint32_t)q->ssrc[s];
            uint32_t w[3];
            w[0] = b0 | b1 << 8 | (miss_sn >> 8) << 16 | (miss_sn & 255u) << 24;
            w[1] = t >> 24 | (t >> 16 & 255u) << 8 | (t >> 8 & 255u) << 16 | (t & 255u) << 24;
            w[2] = ss >> 24 | (ss >> 16 & 255u) << 8 | (ss >> 8 & 255u) << 16 | (ss & 255u) << 24;
            lc3r_header_out(q->ring, slot, w);
            q->rec_dg_offsets[f] = slot; q->rec_dg_sizes[f] = LC3R_FIXED + (int32_t)rl; q->rec_seq[f] = (int32_t)miss_sn;
        }
    }
    if (st) { q->rec_dg_offsets[f] = 0; q->rec_dg_sizes[f] = 0; q->rec_seq[f] = 0; }
    if (q->status) q->status[f] = (uint8_t)st;
    return st;
}

/* one encode call: every pointer but the struct itself is a device pointer */
typedef struct {
    int32_t device, sync;
    lc3fec_enc_in in;
    lc3fec_enc_out out;
    void* work; void* hip_stream;
} lc3fec_encode_call;
/* one recover call */
typedef struct {
    int32_t device, sync;
    lc3fec_rec_io io;
    int32_t* stats;
    void* work; void* hip_stream;
} lc3fec_recover_call;

#ifdef __cplusplus
extern "C" {
#endif
/* queue the kernels on q->hip_stream; wait for them only with q->sync.  0, or 1 where nothing was queued */
int lc3fec_encode_run(const lc3fec_encode_call* q);
int lc3fec_recover_run(const lc3fec_recover_call* q);
/* launches of an FEC kernel by this process, by the kernel's symbol name in the code object; -1 for a name the library does not hold */
long long lc3fec_launch_count(const char* kernel);
#ifdef __cplusplus
}
#endif
#endif
