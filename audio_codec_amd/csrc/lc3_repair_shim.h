/* lc3_repair_shim.h -- generic FEC, repair across calls (include/lc3plus_batch.h "Generic FEC", REPAIR: lc3plus_dec_batch_fec_repair, lc3plus_plan_fec_repair): what
 * the host C code (lc3_packet.c) and the sibling library that holds the repair kernels (lc3_repair.hip -> liblc3plus_repair_hip.so) share.  The rule - which item is
 * usable, the heads, the distance, expiry, admission, the verdict of a stored FEC cell against the media history, the rebuilt header - is one text for the host
 * plan and the kernels: every step below is what one lane does, and the plan runs the lanes one after the other.  The two differ in how payload bytes move (plain
 * bytes on the host, lc3fec_xor_store of lc3_fec_xor.inc on the device) and in lc3rep_min / lc3rep_max, which are atomics on the device.  The item
 * checks, the FEC header and the byte fetches are lc3_fec_shim.h's and lc3_rtp_shim.h's, by inclusion.  The lc3rep_* functions at the end are the sibling's whole
 * C ABI. */
#ifndef LC3_REPAIR_SHIM_H
#define LC3_REPAIR_SHIM_H
#include "lc3_fec_shim.h"

/* LC3PLUS_FEC_REPAIR_STATE_WORDS and the statuses behind LC3PLUS_FEC_OVERFLOW of include/lc3plus_batch.h */
enum { LC3REP_STATE_WORDS = 4, LC3REP_ST_FLAGS = 0, LC3REP_ST_HEAD = 1 };
enum { LC3REP_STORED = 0, LC3REP_STALE = 10, LC3REP_DUPLICATE = 11, LC3REP_OVERSIZE = 12, LC3REP_EXPIRED = 13, LC3REP_TWIN = 14, LC3REP_STATUSES = 15 };
enum { LC3REP_MED = 0, LC3REP_FEC = 1, LC3REP_MAX_PASSES = 4, LC3REP_MIN_MED = 16, LC3REP_MAX_MED = 1024, LC3REP_MIN_CELLS = 4, LC3REP_MAX_CELLS = 256 };
/* LC3REP_COPY_LANES lanes copy a stored item, a wave (LC3FEC_REC_LANES) rebuilds a packet */
enum { LC3REP_THREADS = 256, LC3REP_COPY_LANES = 8, LC3REP_PROG_WORDS = 8 };
/* what a verdict leaves in the workspace for a cell that rebuilds nothing */
#define LC3REP_NONE (-1)

/* what a repair call reads and writes (may be NULL: item_status, fec_status, stats; the media arrays with n_items 0, the FEC arrays with n_fec 0) */
typedef struct {
    uint8_t* ring; const long long* dg_offsets; const int32_t* dg_sizes; const int32_t* stream; const int32_t* seq;
    const int32_t* fec_stream; const long long* fec_offsets; const int32_t* fec_num_bytes; const int32_t* fec_seq; const int32_t* ssrc;
    int32_t* med_seq; int32_t* med_size; uint8_t* fec_store; int32_t* cell_seq; int32_t* cell_size; uint8_t* cell_status; int32_t* state;
    long long* rec_dg_offsets; int32_t* rec_dg_sizes; int32_t* rec_seq; uint8_t* item_status; uint8_t* fec_status; int32_t* stats;
    long long ring_capacity, n_items, n_fec, med_offset;
    int32_t n_streams, med_slots, med_stride, fec_slots, fec_stride, passes;
} lc3rep_io;

/* The workspace, int32 words in this order: prog [LC3REP_PROG_WORDS], prog[p] nonzero where pass p has a cell that rebuilds (prog[0]: always); per kind and
 * stream first (the lowest usable item), dist (the largest step ahead of the base), head and valid (the state after the call); mclaim [n_streams][H] and fclaim
 * [n_streams][P], the lowest item that claims a slot and after the settle step the item stored there in this call or LC3REP_NONE; tclaim [n_streams][H], the lowest
 * cell that rebuilds into a media slot; verdict [n_streams][P], the number a cell rebuilds in the running pass or LC3REP_NONE */
typedef struct { int32_t* prog; int32_t* first; int32_t* dist; int32_t* head; int32_t* valid; int32_t* mclaim; int32_t* fclaim; int32_t* tclaim; int32_t* verdict; } lc3rep_work;
static inline LC3FEC_HD long long lc3rep_work_words(long long n, long long H, long long P) { return LC3REP_PROG_WORDS + 8 * n + 2 * n * H + 2 * n * P; }
static inline LC3FEC_HD long long lc3rep_work_bytes(long long n, long long H, long long P) { return (4 * lc3rep_work_words(n, H, P) + 7) & ~7LL; }
/* the words the fill step sets to LC3FEC_NO_ENTRY (first and the claims) lie in [8, 8 + 2n) and behind 8 + 8n, less the verdicts */
static inline LC3FEC_HD lc3rep_work lc3rep_work_of(void* work, long long n, long long H, long long P)
{
    lc3rep_work w;
    w.prog = (int32_t*)work; w.first = w.prog + LC3REP_PROG_WORDS; w.dist = w.first + 2 * n; w.head = w.dist + 2 * n; w.valid = w.head + 2 * n;
    w.mclaim = w.valid + 2 * n; w.fclaim = w.mclaim + n * H; w.tclaim = w.fclaim + n * P; w.verdict = w.tclaim + n * H;
    return w;
}

/* the lowest, the largest: a plain update where the steps run one after the other, an integer atomic among the lanes of a kernel */
#if defined(__HIP_DEVICE_COMPILE__)
static inline __device__ void lc3rep_min(int32_t* p, int32_t v) { atomicMin(p, v); }
static inline __device__ void lc3rep_max(int32_t* p, int32_t v) { atomicMax(p, v); }
#else
static inline void lc3rep_min(int32_t* p, int32_t v) { if (v < *p) *p = v; }
static inline void lc3rep_max(int32_t* p, int32_t v) { if (v > *p) *p = v; }
#endif

/* 16-bit serial arithmetic: d(a, b) = (int16)(a - b); a number is behind a window of `slots` under head h where d(h, sn) >= slots, ahead of it where d(sn, h) > 0 */
static inline LC3FEC_HD int lc3rep_d(uint32_t a, uint32_t b) { return (int)(int16_t)(uint16_t)(a - b); }
static inline LC3FEC_HD int lc3rep_behind(uint32_t h, uint32_t sn, int slots) { return lc3rep_d(h, sn) >= slots; }
static inline LC3FEC_HD int lc3rep_ahead(uint32_t h, uint32_t sn) { return lc3rep_d(sn, h) > 0; }
/* slot (s, j) of the media history in the ring, cell (s, j) of the FEC store */
static inline LC3FEC_HD long long lc3rep_slot_at(const lc3rep_io* q, long long k) { return q->med_offset + k * q->med_stride; }
static inline LC3FEC_HD long long lc3rep_cell_at(const lc3rep_io* q, long long c) { return c * q->fec_stride; }

/* ---- step 1: usable items.  An item of the call is e in [0, n_items + n_fec): the media items first ---- */
typedef struct { int32_t kind, s, code, size; uint32_t sn; long long idx, off; } lc3rep_item;
/* the FEC items of a call as lc3fec_item_header reads them */
static inline LC3FEC_HD lc3fec_rec_io lc3rep_fec_items(const lc3rep_io* q)
{
    lc3fec_rec_io r = {q->ring, 0, 0, 0, 0, q->fec_stream, q->fec_offsets, q->fec_num_bytes, 0, 0, 0, 0, 0, q->ring_capacity, 0, q->n_fec, 0, 0, q->n_streams, 0};
    return r;
}
/* a datagram that holds a byte of the media history: the call would read it while it writes it, so such an item is RANGE like one outside the ring */
static inline LC3FEC_HD int lc3rep_in_history(const lc3rep_io* q, long long off, int32_t size)
{
    const long long end = q->med_offset + (long long)q->n_streams * q->med_slots * q->med_stride;
    return size > 0 && off < end && off > q->med_offset - size;
}
/* item e with code 0 where it is usable, else the status it gets: a media item DROPPED (stream outside [0, n_streams)), RANGE (outside the ring, or inside the
 * history), SHORT (fewer than 12 bytes), OVERSIZE (more than med_stride), in this order; an FEC item the checks 1 ... 5 of lc3fec_item_header - RANGE also inside
 * the history - then OVERSIZE (more than fec_stride) */
static inline LC3FEC_HD lc3rep_item lc3rep_item_of(const lc3rep_io* q, long long e)
{
    lc3rep_item it;
    it.kind = e >= q->n_items ? LC3REP_FEC : LC3REP_MED;
    it.code = 0;
    if (it.kind == LC3REP_MED) {
        it.idx = e; it.s = q->stream[e]; it.off = q->dg_offsets[e]; it.size = q->dg_sizes[e]; it.sn = (uint32_t)q->seq[e] & 0xFFFFu;
        if (it.s < 0 || it.s >= q->n_streams) it.code = LC3FEC_DROPPED;
        else if (it.off < 0 || it.size < 0 || it.off > q->ring_capacity - it.size || lc3rep_in_history(q, it.off, it.size)) it.code = LC3FEC_RANGE;
        else if (it.size < LC3R_FIXED) it.code = LC3FEC_SHORT;
        else if (it.size > q->med_stride) it.code = LC3REP_OVERSIZE;
    } else {
        const lc3fec_rec_io r = lc3rep_fec_items(q);
        lc3fec_item h;
        it.idx = e - q->n_items; it.s = q->fec_stream[it.idx]; it.off = q->fec_offsets[it.idx]; it.size = q->fec_num_bytes[it.idx];
        it.sn = (uint32_t)q->fec_seq[it.idx] & 0xFFFFu;
        it.code = lc3fec_item_header(&r, it.idx, &h);
        if (it.code != LC3FEC_DROPPED && it.code != LC3FEC_RANGE && lc3rep_in_history(q, it.off, it.size)) it.code = LC3FEC_RANGE;
        if (!it.code && it.size > q->fec_stride) it.code = LC3REP_OVERSIZE;
    }
    return it;
}
static inline LC3FEC_HD int lc3rep_slots(const lc3rep_io* q, int kind) { return kind == LC3REP_FEC ? q->fec_slots : q->med_slots; }

/* ---- step 2: heads ---- */
static inline LC3FEC_HD int lc3rep_old_valid(const lc3rep_io* q, int s, int kind) { return q->state[(size_t)s * LC3REP_STATE_WORDS + LC3REP_ST_FLAGS] >> kind & 1; }
/* the first-index step for item e */
static inline LC3FEC_HD void lc3rep_first_step(const lc3rep_io* q, const lc3rep_work* w, long long e)
{
    const lc3rep_item it = lc3rep_item_of(q, e);
    if (!it.code) lc3rep_min(w->first + (size_t)it.kind * q->n_streams + it.s, (int32_t)it.idx);
}
/* the base of a stream's kind: its head, or without one the number of its lowest usable item.  -> 0 where it has neither */
static inline LC3FEC_HD int lc3rep_base(const lc3rep_io* q, const lc3rep_work* w, int s, int kind, uint32_t* base)
{
    if (lc3rep_old_valid(q, s, kind)) { *base = (uint32_t)q->state[(size_t)s * LC3REP_STATE_WORDS + LC3REP_ST_HEAD + kind] & 0xFFFFu; return 1; }
    const int32_t i = w->first[(size_t)kind * q->n_streams + s];
    if (i == LC3FEC_NO_ENTRY) return 0;
    *base = (uint32_t)(kind == LC3REP_FEC ? q->fec_seq[i] : q->seq[i]) & 0xFFFFu;
    return 1;
}
/* the distance step for item e, behind the first-index step */
static inline LC3FEC_HD void lc3rep_dist_step(const lc3rep_io* q, const lc3rep_work* w, long long e)
{
    const lc3rep_item it = lc3rep_item_of(q, e);
    uint32_t base = 0;
    if (it.code || !lc3rep_base(q, w, it.s, it.kind, &base)) return;
    const int d = lc3rep_d(it.sn, base);
    if (d > 0) lc3rep_max(w->dist + (size_t)it.kind * q->n_streams + it.s, d);
}
/* the head of a stream's kind after the call, behind the distance step.  -> 0 where the kind stays without one */
static inline LC3FEC_HD int lc3rep_new_head(const lc3rep_io* q, const lc3rep_work* w, int s, int kind, uint32_t* head)
{
    uint32_t base = 0;
    if (!lc3rep_base(q, w, s, kind, &base)) return 0;
    *head = (base + (uint32_t)w->dist[(size_t)kind * q->n_streams + s]) & 0xFFFFu;
    return 1;
}

/* ---- step 4, first half: the claim of item e on its slot ---- */
static inline LC3FEC_HD void lc3rep_claim_step(const lc3rep_io* q, const lc3rep_work* w, long long e)
{
    const lc3rep_item it = lc3rep_item_of(q, e);
    uint32_t head = 0;
    if (it.code || !lc3rep_new_head(q, w, it.s, it.kind, &head)) return;
    const int slots = lc3rep_slots(q, it.kind);
    if (((head - it.sn) & 0xFFFFu) >= (uint32_t)slots) return;
    lc3rep_min((it.kind == LC3REP_FEC ? w->fclaim : w->mclaim) + (size_t)it.s * slots + (it.sn & (uint32_t)(slots - 1)), (int32_t)it.idx);
}

/* a stored FEC cell's header, as lc3fec_item_header reads an item's (the checks were made when it was admitted) */
static inline LC3FEC_HD void lc3rep_cell_header(const lc3rep_io* q, long long c, lc3fec_item* h)
{
    const long long off = lc3rep_cell_at(q, c);
    uint32_t w[3];
    lc3r_fetch12(q->fec_store, off, w);
    h->b0 = w[0] >> 24; h->b1 = w[0] >> 16 & 255u; h->sn = w[0] & 0xFFFFu; h->ts = w[1]; h->len = w[2] >> 16; h->plen = w[2] & 0xFFFFu;
    const int L = h->b0 >> 6 & 1;
    h->hl = L ? LC3FEC_HEADER_LONG : LC3FEC_HEADER;
    h->mask = (unsigned long long)lc3r_fetch_be16(q->fec_store, off + 12) << 32;
    if (L) h->mask |= lc3fec_fetch_be32(q->fec_store, off + 14);
}

/* ---- steps 3 and 4: the settle step of slot c of a kind: expiry, the claim's outcome, the metadata; slot 0 of a stream also leaves its head in the workspace.
 * Behind it the claim word of the slot is the item stored there in this call, or LC3REP_NONE ---- */
static inline LC3FEC_HD void lc3rep_settle_step(const lc3rep_io* q, const lc3rep_work* w, int kind, long long c)
{
    const int slots = lc3rep_slots(q, kind), s = (int)(c / slots);
    uint32_t head = 0;
    const int valid = lc3rep_new_head(q, w, s, kind, &head);
    if (c == (long long)s * slots) { w->head[(size_t)kind * q->n_streams + s] = (int32_t)head; w->valid[(size_t)kind * q->n_streams + s] = valid; }
    int32_t* claim = (kind == LC3REP_FEC ? w->fclaim : w->mclaim) + c;
    if (!valid) { *claim = LC3REP_NONE; return; }                       /* no stored packet, no usable item: the arrays stay as they are */
    int32_t* seq = (kind == LC3REP_FEC ? q->cell_seq : q->med_seq) + c;
    int32_t* size = (kind == LC3REP_FEC ? q->cell_size : q->med_size) + c;
    int live = lc3rep_old_valid(q, s, kind) && *size > 0;
    if (live && ((head - (uint32_t)*seq) & 0xFFFFu) >= (uint32_t)slots) live = 0;
    if (live && kind == LC3REP_FEC) {                                   /* a cell all of whose numbers lie behind the media window */
        uint32_t mh = 0;
        if (lc3rep_new_head(q, w, s, LC3REP_MED, &mh)) {
            lc3fec_item h;
            lc3rep_cell_header(q, c, &h);
            int reachable = 0;
            for (int i = 0; i < LC3FEC_MAX_BITS; i++)
                if ((h.mask >> (LC3FEC_MAX_BITS - 1 - i) & 1) && !lc3rep_behind(mh, (h.sn + (uint32_t)i) & 0xFFFFu, q->med_slots)) reachable = 1;
            live = reachable;
        }
    }
    if (live) { *claim = LC3REP_NONE; return; }
    const int32_t i = *claim;
    if (i == LC3FEC_NO_ENTRY) {
        *seq = 0; *size = 0; *claim = LC3REP_NONE;
        if (kind == LC3REP_FEC) q->cell_status[c] = 0;
        return;
    }
    if (kind == LC3REP_FEC) { *seq = (int32_t)((uint32_t)q->fec_seq[i] & 0xFFFFu); *size = q->fec_num_bytes[i]; q->cell_status[c] = LC3FEC_MISSING; }
    else { *seq = (int32_t)((uint32_t)q->seq[i] & 0xFFFFu); *size = q->dg_sizes[i]; }
}

/* ---- step 4, second half: where item e went, behind the settle step.  -> its status; STORED: *slot is its slot or cell ---- */
static inline LC3FEC_HD int lc3rep_place_step(const lc3rep_io* q, const lc3rep_work* w, const lc3rep_item* it, long long* slot)
{
    if (it->code) return it->code;
    const int slots = lc3rep_slots(q, it->kind);
    const uint32_t head = (uint32_t)w->head[(size_t)it->kind * q->n_streams + it->s];
    if (((head - it->sn) & 0xFFFFu) >= (uint32_t)slots) return LC3REP_STALE;
    *slot = (long long)it->s * slots + (it->sn & (uint32_t)(slots - 1));
    return (it->kind == LC3REP_FEC ? w->fclaim : w->mclaim)[*slot] == (int32_t)it->idx ? LC3REP_STORED : LC3REP_DUPLICATE;
}

/* ---- step 5: a pass ---- */
/* the member sn of stream s in the media history: -> 1, its slot in *k; 0 where it is missing */
static inline LC3FEC_HD int lc3rep_lookup(const lc3rep_io* q, const lc3rep_work* w, int s, uint32_t sn, long long* k)
{
    *k = (long long)s * q->med_slots + (sn & (uint32_t)(q->med_slots - 1));
    return w->valid[(size_t)LC3REP_MED * q->n_streams + s] && q->med_size[*k] > 0 && ((uint32_t)q->med_seq[*k] & 0xFFFFu) == sn;
}
/* the recovery fields of the stored member in slot k: byte 0's low six bits and byte 1, the timestamp, the length */
static inline LC3FEC_HD void lc3rep_member_fields(const lc3rep_io* q, long long k, uint32_t* hdr, uint32_t* ts, uint32_t* len)
{
    const long long at = lc3rep_slot_at(q, k);
    *hdr = (lc3r_fetch_byte(q->ring, at) & 0x3Fu) | lc3r_fetch_byte(q->ring, at + 1) << 8;
    *ts = lc3fec_fetch_be32(q->ring, at + 4);
    *len = (uint32_t)(q->med_size[k] - LC3R_FIXED) & 0xFFFFu;
}
/* a carried cell that settles counts in stats under its new status; the cells stored in this call are counted with their items */
static inline LC3FEC_HD int lc3rep_carried(const lc3rep_work* w, long long c) { return w->fclaim[c] < 0; }
/* The verdict step of cell c in pass p (1 ...), against the history as the pass found it.  -> the final status the cell takes, LC3FEC_MISSING where it stays open,
 * LC3FEC_RECOVERED where it rebuilds (its number in verdict[c], its claim on the slot made; the rebuild step finishes it), -1 for a cell that is not open */
static inline LC3FEC_HD int lc3rep_verdict_step(const lc3rep_io* q, const lc3rep_work* w, int p, long long c)
{
    const int s = (int)(c / q->fec_slots);
    w->verdict[c] = LC3REP_NONE;
    if (!w->valid[(size_t)LC3REP_FEC * q->n_streams + s] || q->cell_size[c] <= 0 || q->cell_status[c] != LC3FEC_MISSING) return -1;
    const int medv = w->valid[(size_t)LC3REP_MED * q->n_streams + s];
    const uint32_t mh = (uint32_t)w->head[(size_t)LC3REP_MED * q->n_streams + s];
    lc3fec_item h;
    lc3rep_cell_header(q, c, &h);
    uint32_t len = 0, miss_sn = 0;                                      /* of the members' fields the verdict needs the lengths alone */
    int missing = 0, behind = 0, wait = 0;
    for (int i = 0; i < LC3FEC_MAX_BITS; i++) {
        if (!(h.mask >> (LC3FEC_MAX_BITS - 1 - i) & 1)) continue;
        const uint32_t sn = (h.sn + (uint32_t)i) & 0xFFFFu;
        long long k = 0;
        if (!lc3rep_lookup(q, w, s, sn, &k)) {
            missing++; miss_sn = sn;
            if (!medv || lc3rep_ahead(mh, sn)) wait++;
            else if (lc3rep_behind(mh, sn, q->med_slots)) behind++;
            continue;
        }
        len ^= (uint32_t)(q->med_size[k] - LC3R_FIXED) & 0xFFFFu;
    }
    const uint32_t rl = h.len ^ len;
    int st;
    if (missing == 0) st = LC3FEC_COMPLETE;
    else if (behind) st = LC3REP_EXPIRED;
    else if (missing > 1 || wait) st = LC3FEC_MISSING;
    else if (rl > h.plen) st = LC3FEC_PARTIAL;
    else if (LC3R_FIXED + (long long)rl > q->med_stride) st = LC3FEC_OVERFLOW;
    else st = LC3FEC_RECOVERED;
    if (st == LC3FEC_RECOVERED) {
        w->verdict[c] = (int32_t)miss_sn;
        lc3rep_min(w->tclaim + (size_t)s * q->med_slots + (miss_sn & (uint32_t)(q->med_slots - 1)), (int32_t)c);
        w->prog[p] = 1;
    } else if (st != LC3FEC_MISSING) q->cell_status[c] = (uint8_t)st;
    return st;
}
/* what the rebuild step of cell c finds: -> LC3FEC_RECOVERED where the cell writes (its header h, the media slot *k, the number *sn), LC3REP_TWIN where a lower
 * cell does, -1 where verdict[c] names no number */
static inline LC3FEC_HD int lc3rep_rebuild_claim(const lc3rep_io* q, const lc3rep_work* w, long long c, lc3fec_item* h, long long* k, uint32_t* sn)
{
    const int32_t v = w->verdict[c];
    if (v < 0) return -1;
    const int s = (int)(c / q->fec_slots);
    *sn = (uint32_t)v;
    *k = (long long)s * q->med_slots + (*sn & (uint32_t)(q->med_slots - 1));
    if (w->tclaim[*k] != (int32_t)c) { q->cell_status[c] = LC3REP_TWIN; return LC3REP_TWIN; }
    lc3rep_cell_header(q, c, h);
    return LC3FEC_RECOVERED;
}
/* the rebuilt packet's twelve header bytes, its records and the cell's status, from the XOR of the present members' fields */
static inline LC3FEC_HD int32_t lc3rep_rebuild_header(const lc3rep_io* q, long long c, const lc3fec_item* h, long long k, uint32_t sn, uint32_t hdr, uint32_t ts, uint32_t len)
{
    const int s = (int)(c / q->fec_slots);
    const uint32_t rl = h->len ^ len, b0 = 0x80u | ((h->b0 ^ hdr) & 0x3Fu), b1 = (h->b1 ^ (hdr >> 8)) & 255u, t = h->ts ^ ts, ss = (uint32_t)q->ssrc[s];
    uint32_t w[3];
    w[0] = b0 | b1 << 8 | (sn >> 8) << 16 | (sn & 255u) << 24;
    w[1] = t >> 24 | (t >> 16 & 255u) << 8 | (t >> 8 & 255u) << 16 | (t & 255u) << 24;
    w[2] = ss >> 24 | (ss >> 16 & 255u) << 8 | (ss >> 8 & 255u) << 16 | (ss & 255u) << 24;
    lc3r_header_out(q->ring, lc3rep_slot_at(q, k), w);
    q->med_seq[k] = (int32_t)sn; q->med_size[k] = LC3R_FIXED + (int32_t)rl;
    q->rec_dg_offsets[c] = lc3rep_slot_at(q, k); q->rec_dg_sizes[c] = LC3R_FIXED + (int32_t)rl; q->rec_seq[c] = (int32_t)sn;
    q->cell_status[c] = LC3FEC_RECOVERED;
    return (int32_t)rl;
}

/* ---- step 6: the report of FEC item f, behind the last pass: the reason it was not stored, or its cell's status ---- */
static inline LC3FEC_HD int lc3rep_report_step(const lc3rep_io* q, const lc3rep_work* w, long long f)
{
    const lc3rep_item it = lc3rep_item_of(q, q->n_items + f);
    long long c = 0;
    int st = lc3rep_place_step(q, w, &it, &c);
    if (st == LC3REP_STORED) st = q->cell_status[c];
    if (q->fec_status) q->fec_status[f] = (uint8_t)st;
    return st;
}
/* ... and the state of stream s: a kind with a head has its bit and its head written, the fourth word is 0; a stream with neither keeps its words */
static inline LC3FEC_HD void lc3rep_state_step(const lc3rep_io* q, const lc3rep_work* w, int s)
{
    const int mv = w->valid[(size_t)LC3REP_MED * q->n_streams + s], fv = w->valid[(size_t)LC3REP_FEC * q->n_streams + s];
    int32_t* st = q->state + (size_t)s * LC3REP_STATE_WORDS;
    if (!mv && !fv) return;
    st[LC3REP_ST_FLAGS] = mv | fv << 1;
    if (mv) st[LC3REP_ST_HEAD + LC3REP_MED] = w->head[(size_t)LC3REP_MED * q->n_streams + s];
    if (fv) st[LC3REP_ST_HEAD + LC3REP_FEC] = w->head[(size_t)LC3REP_FEC * q->n_streams + s];
    st[3] = 0;
}

/* one repair call: every pointer but the struct itself is a device pointer */
typedef struct {
    int32_t device, sync;
    lc3rep_io io;
    void* work; void* hip_stream;
} lc3rep_call;

#ifdef __cplusplus
extern "C" {
#endif
/* queue the kernels on q->hip_stream; wait for them only with q->sync.  0, or 1 where nothing was queued */
int lc3rep_repair_run(const lc3rep_call* q);
/* launches of a repair kernel by this process, by the kernel's symbol name in the code object; -1 for a name the library does not hold */
long long lc3rep_launch_count(const char* kernel);
#ifdef __cplusplus
}
#endif
#endif
