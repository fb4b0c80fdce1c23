/* lc3_packet.c -- host side (plain C) of the packet layer of include/lc3plus_batch.h: the frame probe, packet ingest and egress, RTP framing, reception
 * reports, Secure RTP in both suites, redundant audio and generic FEC.  Per call: the checks, the rule on the host (lc3plus_plan_*) on the text the kernels
 * run, and the entry points of a batch, which hand the call to the sibling library that holds its kernels (DESIGN.md "Sibling libraries").
 *
 * Two rules hold throughout this file:
 *   - Of a batch the layer sees its view and nothing else (lc3_batch_view.h): no definition of a batch struct is included here.
 *   - A call's parameter list is written once, X_PARAMS (the header's order, behind the batch and in front of hip_stream and sync), and so is the initialiser
 *     of its X_args struct from those names, X_ARGS; every plan and entry point of the call is declared and filled with the two.  The prototypes written out in
 *     include/lc3plus_batch.h are what the compiler checks each of them against.
 */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE                 /* dladdr: the sibling libraries are loaded from this library's directory */
#endif
#include <dlfcn.h>
#include <limits.h>
#include <pthread.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/lc3.h"
#include "../../include/lc3plus_batch.h"
#include "lc3_shim.h"
#include "lc3_probe_shim.h"
#include "lc3_ingest_shim.h"
#include "lc3_egress_shim.h"
#include "lc3_rtp_shim.h"
#include "lc3_rtcp_shim.h"
#include "lc3_srtp_shim.h"
#include "lc3_gcm_shim.h"
#include "lc3_red_shim.h"
#include "lc3_fec_shim.h"
#include "lc3_repair_shim.h"
#include "lc3_batch_view.h"

#define IMIN(a, b) ((a) < (b) ? (a) : (b))

/* ---- the sibling libraries (DESIGN.md "Sibling libraries"): the kernels of every call below lie in a library of their own beside this one ---- */
enum { SIB_PROBE, SIB_INGEST, SIB_EGRESS, SIB_RTP, SIB_RTCP, SIB_SRTP, SIB_GCM, SIB_RED, SIB_FEC, SIB_REPAIR, SIB_COUNT };
/* a row: the file, its one or two entry points, and where they go.  fn holds either all of them or none */
static struct { const char* file; const char* sym[2]; int tried; void* fn[2]; } siblings[SIB_COUNT] = {
    [SIB_PROBE] = {"liblc3plus_probe_hip.so", {"lc3probe_run", NULL}, 0, {NULL, NULL}},
    [SIB_INGEST] = {"liblc3plus_ingest_hip.so", {"lc3ingest_run", NULL}, 0, {NULL, NULL}},
    [SIB_EGRESS] = {"liblc3plus_egress_hip.so", {"lc3egress_run", NULL}, 0, {NULL, NULL}},
    [SIB_RTP] = {"liblc3plus_rtp_hip.so", {"lc3rtp_parse_run", "lc3rtp_stamp_run"}, 0, {NULL, NULL}},
    [SIB_RTCP] = {"liblc3plus_rtcp_hip.so", {"lc3rtcp_stats_run", NULL}, 0, {NULL, NULL}},
    [SIB_SRTP] = {"liblc3plus_srtp_hip.so", {"lc3srtp_protect_run", "lc3srtp_unprotect_run"}, 0, {NULL, NULL}},
    [SIB_GCM] = {"liblc3plus_gcm_hip.so", {"lc3gcm_protect_run", "lc3gcm_unprotect_run"}, 0, {NULL, NULL}},
    [SIB_RED] = {"liblc3plus_red_hip.so", {"lc3red_pack_run", "lc3red_unpack_run"}, 0, {NULL, NULL}},
    [SIB_FEC] = {"liblc3plus_fec_hip.so", {"lc3fec_encode_run", "lc3fec_recover_run"}, 0, {NULL, NULL}},
    [SIB_REPAIR] = {"liblc3plus_repair_hip.so", {"lc3rep_repair_run", NULL}, 0, {NULL, NULL}},
};
static pthread_mutex_t sibling_mu = PTHREAD_MUTEX_INITIALIZER;
/* The entry points of a sibling, or NULL where the library is missing or lacks one of them.  The file is looked for once per process, on the first call that needs
 * it, in the directory this library lies in; the first failure says so on stderr, every later call fails silently. */
static void* const* sibling_load(int which)
{
    pthread_mutex_lock(&sibling_mu);
    if (!siblings[which].tried) {
        siblings[which].tried = 1;
        const char* const file = siblings[which].file;
        Dl_info di;
        char path[4096];
        const char* why = "this library's own path is unknown or too long";
        void* h = NULL;
        if (dladdr((void*)&sibling_load, &di) && di.dli_fname) {
            const char* slash = strrchr(di.dli_fname, '/');
            const size_t dir = slash ? (size_t)(slash - di.dli_fname) + 1 : 0;
            if (dir + strlen(file) < sizeof path) {
                memcpy(path, di.dli_fname, dir);
                strcpy(path + dir, file);
                h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
                if (!h) why = dlerror();
            }
        }
        void* fn[2] = {NULL, NULL};
        int ok = h != NULL;
        for (int k = 0; ok && k < 2 && siblings[which].sym[k]; k++) { fn[k] = dlsym(h, siblings[which].sym[k]); if (!fn[k]) { ok = 0; why = dlerror(); } }
        if (ok) memcpy(siblings[which].fn, fn, sizeof fn);
        else fprintf(stderr, "lc3plus_hip: the sibling library %s cannot be used: %s\n", file, why ? why : "an entry point is missing");
    }
    void* const* fn = siblings[which].fn[0] ? siblings[which].fn : NULL;
    pthread_mutex_unlock(&sibling_mu);
    return fn;
}
/* a batch's device and its context's own stream (want_stream: an encoder's own stream is created where no call has needed it yet) */
static int batch_device(lc3host_view v, int want_stream, int32_t* device, void** own)
{
    if (v.decoder) {
        const lc3d_plan* plan = NULL; const lc3d_dchan* tab = NULL; int tab_n = 0;
        return lc3hip_dec_probe_args(v.dev, device, &plan, &tab, &tab_n, own);
    }
    return lc3hip_stream_args(v.dev, want_stream, device, own);
}
/* How every call into a sibling begins, behind its argument checks: the batch's device and the stream the call runs on - the caller's, or the batch's own;
 * nonzero where the batch refuses */
static int sibling_call(lc3host_view v, void* hip_stream, int32_t* device, void** stream)
{
    void* own = NULL;
    if (batch_device(v, !hip_stream, device, &own)) return 1;
    *stream = hip_stream ? hip_stream : own;
    return 0;
}
/* and how it ends, as an LC3_Error: entry point k of the sibling, called through a pointer of its own type (T: its call struct) on the filled struct q;
 * LC3_ERROR where the library cannot be used or the entry point refuses */
#define SIBLING_ENTER(T, which, k, q) (sibling_load(which) && !((int (*)(const T*))siblings[which].fn[k])(q) ? LC3_OK : LC3_ERROR)
/* the whole tail of an entry point whose struct q (all else filled) takes the two as device and hip_stream: every call's but the probe's */
#define SIBLING_RUN(T, which, k, v, hip_stream, q) (sibling_call(v, hip_stream, &(q)->device, &(q)->hip_stream) ? LC3_ERROR : SIBLING_ENTER(T, which, k, q))
/* The two entry points of a call that a batch of either kind makes, lc3plus_{enc,dec}_batch_NAME, from one text: they differ in the view they take and in
 * nothing else.  PARAMS, args_t, ARGS: the call's list, its struct and the struct's initialiser; QUEUE: the call of the function both end in, with the
 * struct a, the view v, hip_stream and sync.  A NULL batch is refused first, before the view is taken */
#define BATCH_TWINS(NAME, PARAMS, args_t, ARGS, QUEUE) \
    LC3_Error lc3plus_enc_batch_##NAME(lc3plus_batch* b, PARAMS, void* hip_stream, int sync) \
    { \
        if (!b) return LC3_NULL_ERROR; \
        const args_t a = ARGS; \
        const lc3host_view v = lc3host_enc_view(b); \
        return QUEUE; \
    } \
    LC3_Error lc3plus_dec_batch_##NAME(lc3plus_dec_batch* b, PARAMS, void* hip_stream, int sync) \
    { \
        if (!b) return LC3_NULL_ERROR; \
        const args_t a = ARGS; \
        const lc3host_view v = lc3host_dec_view(b); \
        return QUEUE; \
    }
/* ---- the frame probe (include/lc3plus_batch.h "Frame probe"; lc3_probe_shim.h; lc3plus_frame_info_side and lc3plus_reject_name are lc3_host.c's) ---- */
LC3_Error lc3plus_dec_batch_probe(lc3plus_dec_batch* b, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes,
                                  int max_frame_bytes, int64_t n_items, int depth, int32_t* info, void* hip_stream, int sync)
{
    if (!b || !frames || !offsets || !num_bytes || !info) return LC3_NULL_ERROR;
    if (n_items <= 0 || max_frame_bytes <= 0 || frames_capacity < 0 || (depth != LC3P_DEPTH_SIDE && depth != LC3P_DEPTH_FULL)) return LC3_ERROR;
    const lc3host_view v = lc3host_dec_view(b);
    lc3probe_call q;
    memset(&q, 0, sizeof q);
    void* own = NULL;
    if (lc3hip_dec_probe_args(v.dev, &q.device, &q.plan, &q.tab, &q.tab_n, &own)) return LC3_ERROR;     /* the probe alone also borrows plan and table */
    q.stream = hip_stream ? hip_stream : own;
    q.channels = v.channels; q.ylen = v.ylen;
    q.frames = frames; q.capacity = (long long)frames_capacity; q.offsets = (const long long*)offsets; q.num_bytes = num_bytes; q.max_bytes = max_frame_bytes;
    q.depth = depth; q.n_items = (long long)n_items; q.info = info; q.sync = sync;
    return SIBLING_ENTER(lc3probe_call, SIB_PROBE, 0, &q);
}
/* ---- packet ingest (include/lc3plus_batch.h "Packet ingest"; lc3_ingest_shim.h) ---- */
/* what both calls take behind n_streams and channels or the batch, in the header's order */
typedef struct {
    int64_t n_items; const int32_t* stream; const int32_t* seq; const int64_t* offsets; const int32_t* num_bytes; const int32_t* info; const int32_t* base;
    const int32_t* floor; int seq_bits; int n_frames; int64_t* out_offsets; int32_t* out_num_bytes; int32_t* cell_item; int32_t* counts; int32_t* next_base;
    int32_t* stats; uint8_t* item_status;
} ingest_args;
#define INGEST_PARAMS \
    int64_t n_items, const int32_t* stream, const int32_t* seq, const int64_t* offsets, const int32_t* num_bytes, const int32_t* info, const int32_t* base, \
    const int32_t* floor, int seq_bits, int n_frames, int64_t* out_offsets, int32_t* out_num_bytes, int32_t* cell_item, int32_t* counts, int32_t* next_base, \
    int32_t* stats, uint8_t* item_status
#define INGEST_ARGS \
    {n_items, stream, seq, offsets, num_bytes, info, base, floor, seq_bits, n_frames, out_offsets, out_num_bytes, cell_item, counts, next_base, stats, item_status}
/* the checks both calls make first, in the header's order */
static LC3_Error ingest_check(const ingest_args* a)
{
    if (!a->stream || !a->seq || !a->offsets || !a->num_bytes || !a->base || !a->out_offsets || !a->out_num_bytes || !a->cell_item || !a->counts) return LC3_NULL_ERROR;
    if (a->n_items <= 0 || a->n_items >= LC3I_MAX_ITEMS || a->n_frames <= 0 || (a->seq_bits != 16 && a->seq_bits != 32)) return LC3_ERROR;
    return LC3_OK;
}
/* the rule on the host: the steps of the kernels (lc3_ingest.inc) one after the other, on the text they run */
LC3_Error lc3plus_plan_ingest(int n_streams, int channels, INGEST_PARAMS)
{
    const ingest_args a = INGEST_ARGS;
    LC3_Error e = ingest_check(&a);
    if (e) return e;
    if (n_streams <= 0 || channels < 1) return LC3_ERROR;
    uint32_t* key = (uint32_t*)cell_item;
    for (size_t c = 0; c < (size_t)n_streams * n_frames; c++) key[c] = LC3I_NO_KEY;
    if (stats) memset(stats, 0, sizeof(int32_t) * LC3I_STATS_WORDS * (size_t)n_streams);
    for (int64_t i = 0; i < n_items; i++) {
        int t = 0, rank = 0;
        const int cls = lc3i_item(stream[i], seq[i], num_bytes[i], info ? info + (size_t)i * channels * LC3I_INFO_WORDS : NULL, channels, n_streams, base, seq_bits,
                                  n_frames, &t, &rank);
        if (cls == 0) { uint32_t* k = key + (size_t)stream[i] * n_frames + t; if (lc3i_key(rank, i) < *k) *k = lc3i_key(rank, i); }
        else if (stats && (cls == LC3I_LATE || cls == LC3I_EARLY)) stats[(size_t)stream[i] * LC3I_STATS_WORDS + (cls == LC3I_LATE ? LC3I_ST_LATE : LC3I_ST_EARLY)]++;
    }
    for (int s = 0; s < n_streams; s++) {
        int top = -1, won = 0;
        for (int t = 0; t < n_frames; t++) {
            const size_t c = (size_t)s * n_frames + t;
            const int32_t w = key[c] == LC3I_NO_KEY ? -1 : (int32_t)(key[c] & LC3I_ITEM_MASK);
            if (w >= 0) { top = t; won++; }
            out_offsets[c] = w >= 0 ? offsets[w] : 0; out_num_bytes[c] = w >= 0 ? num_bytes[w] : 0; cell_item[c] = w;
        }
        counts[s] = lc3i_count(floor ? floor[s] : 0, n_frames, top);
        if (next_base) next_base[s] = lc3i_next_base(base[s], counts[s], seq_bits);
        if (stats) { stats[(size_t)s * LC3I_STATS_WORDS + LC3I_ST_COUNT] = counts[s]; stats[(size_t)s * LC3I_STATS_WORDS + LC3I_ST_GAPS] = counts[s] - won; }
    }
    if (item_status)
        for (int64_t i = 0; i < n_items; i++) {
            int t = 0, rank = 0;
            int st = lc3i_item(stream[i], seq[i], num_bytes[i], info ? info + (size_t)i * channels * LC3I_INFO_WORDS : NULL, channels, n_streams, base, seq_bits,
                               n_frames, &t, &rank);
            if (st == 0) st = lc3i_candidate_status(rank, i, cell_item[(size_t)stream[i] * n_frames + t]);
            item_status[i] = (uint8_t)st;
        }
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_ingest(lc3plus_dec_batch* b, INGEST_PARAMS, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    const ingest_args a = INGEST_ARGS;
    LC3_Error e = ingest_check(&a);
    if (e) return e;
    const lc3host_view v = lc3host_dec_view(b);
    lc3ingest_call q;
    memset(&q, 0, sizeof q);
    q.n_streams = v.n_streams; q.channels = v.channels; q.seq_bits = seq_bits; q.n_frames = n_frames; q.sync = sync; q.n_items = (long long)n_items;
    q.stream = stream; q.seq = seq; q.offsets = (const long long*)offsets; q.num_bytes = num_bytes; q.info = info; q.base = base; q.floor = floor;
    q.out_offsets = (long long*)out_offsets; q.out_num_bytes = out_num_bytes; q.cell_item = cell_item; q.counts = counts; q.next_base = next_base; q.stats = stats;
    q.item_status = item_status;
    return SIBLING_RUN(lc3ingest_call, SIB_INGEST, 0, v, hip_stream, &q);
}
/* ---- packet egress (include/lc3plus_batch.h "Packet egress"; lc3_egress_shim.h) ---- */
/* what every egress call takes behind its batch, in the header's order */
typedef struct {
    int n_frames; const void* frames; int64_t frames_capacity; const int64_t* offsets; const int32_t* num_bytes; int max_frame_bytes;
    const uint8_t* flags; int skip_mask; const int32_t* counts;
    int n_routes; const int32_t* route_src; const int32_t* seq_base; int seq_bits; int order;
    void* wire; int64_t wire_capacity; int header_room; int align;
    int32_t* pkt_route; int32_t* pkt_seq; int32_t* pkt_frame; int64_t* pkt_offset; int32_t* pkt_size; uint8_t* pkt_flags;
    int64_t* n_packets; int64_t* wire_total; int32_t* next_seq; int32_t* stats; uint8_t* cell_status;
    void* work;
} egress_args;
#define EGRESS_PARAMS \
    int n_frames, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes, int max_frame_bytes, \
    const uint8_t* flags, int skip_mask, const int32_t* counts, \
    int n_routes, const int32_t* route_src, const int32_t* seq_base, int seq_bits, int order, \
    void* wire, int64_t wire_capacity, int header_room, int align, \
    int32_t* pkt_route, int32_t* pkt_seq, int32_t* pkt_frame, int64_t* pkt_offset, int32_t* pkt_size, uint8_t* pkt_flags, \
    int64_t* n_packets, int64_t* wire_total, int32_t* next_seq, int32_t* stats, uint8_t* cell_status, \
    void* work
#define EGRESS_ARGS \
    {n_frames, frames, frames_capacity, offsets, num_bytes, max_frame_bytes, flags, skip_mask, counts, n_routes, route_src, seq_base, seq_bits, order, \
     wire, wire_capacity, header_room, align, pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, pkt_flags, n_packets, wire_total, next_seq, \
     stats, cell_status, work}
/* the checks every call makes first, in the header's order; n_streams < 0: not known yet (the batch is looked at behind them) */
static LC3_Error egress_check(const egress_args* a, int n_streams)
{
    if (!a->frames || !a->offsets || !a->num_bytes || !a->seq_base || !a->pkt_route || !a->pkt_seq || !a->pkt_frame || !a->pkt_offset || !a->pkt_size ||
        !a->n_packets || !a->work)
        return LC3_NULL_ERROR;
    if (a->n_frames <= 0 || a->n_routes <= 0 || (int64_t)a->n_routes * a->n_frames >= LC3E_MAX_CELLS || a->max_frame_bytes <= 0 || a->frames_capacity < 0 ||
        a->wire_capacity < 0)
        return LC3_ERROR;
    if ((a->order != LC3E_STREAM_MAJOR && a->order != LC3E_FRAME_MAJOR) || (a->seq_bits != 16 && a->seq_bits != 32)) return LC3_ERROR;
    if (a->header_room < 0 || a->header_room > INT32_MAX - LC3E_MAX_ALIGN - a->max_frame_bytes) return LC3_ERROR;
    if (a->align < 1 || a->align > LC3E_MAX_ALIGN || (a->align & (a->align - 1))) return LC3_ERROR;
    if (!a->wire && (a->header_room != 0 || a->align != 1)) return LC3_ERROR;
    if (n_streams >= 0 && !a->route_src && a->n_routes != n_streams) return LC3_ERROR;
    if ((uintptr_t)a->work & 7) return LC3_ERROR;
    return LC3_OK;
}
int64_t lc3plus_egress_work_bytes(int n_routes, int n_frames)
{
    if (n_routes <= 0 || n_frames <= 0 || (int64_t)n_routes * n_frames >= LC3E_MAX_CELLS) return 0;
    return lc3e_work_bytes((long long)n_routes * n_frames);
}
/* the copy kernel's runs on the host, one after the other */
static void egress_copy(uint8_t* dst, const uint8_t* src, int n)
{
    const lc3e_copy_plan c = lc3e_copy_layout((uintptr_t)dst, n);
    const int runs[5] = {c.hb, 4 * c.hd, 16 * c.pieces, 4 * c.td, c.tb};
    for (int k = 0, at = 0; k < 5; at += runs[k++]) memcpy(dst + at, src + at, (size_t)runs[k]);
}
/* the rule on the host: the steps of the kernels (lc3_egress.inc) one after the other, on the text they run and over the same workspace */
LC3_Error lc3plus_plan_egress(int n_streams, EGRESS_PARAMS, void* hip_stream, int sync)
{
    const egress_args a = EGRESS_ARGS;
    LC3_Error e = egress_check(&a, -1);
    if (e) return e;
    if (n_streams <= 0) return LC3_ERROR;
    e = egress_check(&a, n_streams);
    if (e) return e;
    const long long n_cells = (long long)n_routes * n_frames, n_tiles = lc3e_tiles(n_cells);
    const int wire_mode = wire != NULL;
    int32_t* word = (int32_t*)work;
    long long* sums = (long long*)((char*)work + lc3e_work_sums(n_cells));
    lc3e_list L = {pkt_route, pkt_seq, pkt_frame, (long long*)pkt_offset, pkt_size, pkt_flags, cell_status, NULL};
    if (!L.status && stats) L.status = (uint8_t*)work + lc3e_work_status(n_cells);
    if (wire_mode) L.from = (long long*)((char*)work + lc3e_work_from(n_cells));
    /* classify */
    for (long long i = 0; i < n_cells; i++) {
        int r, t;
        lc3e_cell_rt(i, n_routes, n_frames, order, &r, &t);
        word[i] = lc3e_cell_word(r, t, n_streams, route_src, counts, n_frames, (const long long*)offsets, num_bytes, flags, max_frame_bytes, frames_capacity, skip_mask);
    }
    /* the tiles' sums, then their bases and the totals */
    for (long long b = 0; b < n_tiles; b++) {
        long long cnt = 0, bytes = 0;
        for (long long i = b * LC3E_TILE; i < n_cells && i < (b + 1) * LC3E_TILE; i++) { cnt += word[i] > 0; bytes += lc3e_advance(word[i], wire_mode, header_room, align); }
        sums[2 * b] = cnt; sums[2 * b + 1] = bytes;
    }
    long long run_c = 0, run_b = 0;
    for (long long b = 0; b < n_tiles; b++) {
        const long long cnt = sums[2 * b], bytes = sums[2 * b + 1];
        sums[2 * b] = run_c; sums[2 * b + 1] = run_b;
        run_c += cnt; run_b += bytes;
    }
    *n_packets = run_c;
    if (wire_total) *wire_total = run_b;
    /* scatter, and the copy of each packet that fits */
    for (long long b = 0; b < n_tiles; b++) {
        long long p = sums[2 * b], run = sums[2 * b + 1];
        for (long long i = b * LC3E_TILE; i < n_cells && i < (b + 1) * LC3E_TILE; i++) {
            int r, t;
            lc3e_cell_rt(i, n_routes, n_frames, order, &r, &t);
            int st = -word[i];
            if (word[i] > 0) {
                const int s = route_src ? route_src[r] : r;
                st = lc3e_emit(&L, p, r, t, s, word[i], run, seq_base, seq_bits, n_frames, (const long long*)offsets, wire_mode, header_room, wire_capacity);
                if (wire_mode && !(st & LC3E_OVERFLOW)) egress_copy((uint8_t*)wire + run + header_room, (const uint8_t*)frames + L.from[p], word[i]);
                p++; run += lc3e_advance(word[i], wire_mode, header_room, align);
            }
            if (L.status) L.status[(size_t)r * n_frames + t] = (uint8_t)st;
        }
    }
    /* the routes */
    if (next_seq || stats)
        for (int r = 0; r < n_routes; r++) {
            int s = 0, sent = 0, holes = 0, over = 0;
            const int c = lc3e_route(route_src, r, n_streams, counts, n_frames, &s);
            if (stats)
                for (int t = 0; t < c; t++) {
                    const int st = L.status[(size_t)r * n_frames + t];
                    sent += (st & LC3E_SENT) != 0; over += (st & LC3E_OVERFLOW) != 0; holes += (st & (LC3E_LOST | LC3E_INVALID | LC3E_SKIPPED)) != 0;
                }
            lc3e_route_out(r, c, sent, holes, over, seq_base, seq_bits, next_seq, stats);
        }
    return LC3_OK;
}
/* both entry points end here: the checks, the one that needs the batch's n_streams behind the others, then the sibling */
static LC3_Error egress_queue(lc3host_view v, const egress_args* a, void* hip_stream, int sync)
{
    LC3_Error e = egress_check(a, -1);
    if (e) return e;
    if (!a->route_src && a->n_routes != v.n_streams) return LC3_ERROR;
    lc3egress_call q;
    memset(&q, 0, sizeof q);
    q.n_streams = v.n_streams; q.n_frames = a->n_frames; q.max_frame_bytes = a->max_frame_bytes; q.skip_mask = a->skip_mask; q.n_routes = a->n_routes;
    q.seq_bits = a->seq_bits; q.order = a->order; q.header_room = a->header_room; q.align = a->align; q.sync = sync;
    q.frames_capacity = (long long)a->frames_capacity; q.wire_capacity = (long long)a->wire_capacity;
    q.frames = a->frames; q.offsets = (const long long*)a->offsets; q.num_bytes = a->num_bytes; q.flags = a->flags; q.counts = a->counts; q.route_src = a->route_src;
    q.seq_base = a->seq_base; q.wire = a->wire;
    q.list.route = a->pkt_route; q.list.seq = a->pkt_seq; q.list.frame = a->pkt_frame; q.list.offset = (long long*)a->pkt_offset; q.list.size = a->pkt_size;
    q.list.flags = a->pkt_flags; q.list.status = a->cell_status;
    q.n_packets = (long long*)a->n_packets; q.wire_total = (long long*)a->wire_total; q.next_seq = a->next_seq; q.stats = a->stats; q.work = a->work;
    return SIBLING_RUN(lc3egress_call, SIB_EGRESS, 0, v, hip_stream, &q);
}
BATCH_TWINS(egress, EGRESS_PARAMS, egress_args, EGRESS_ARGS, egress_queue(v, &a, hip_stream, sync))
/* ---- RTP framing (include/lc3plus_batch.h "RTP framing"; lc3_rtp_shim.h) ---- */
/* what a parse call takes behind its batch, in the header's order */
typedef struct {
    int64_t n_items; const void* ring; int64_t ring_capacity; const int64_t* dg_offsets; const int32_t* dg_sizes;
    int n_ssrc; const int32_t* ssrc_key; const int32_t* ssrc_stream; const int32_t* payload_type; int payload_room;
    int32_t* stream; int32_t* seq; int64_t* offsets; int32_t* num_bytes; int32_t* timestamp; uint8_t* marker; uint8_t* status; int32_t* stats;
} rtp_parse_args;
#define RTP_PARSE_PARAMS \
    int64_t n_items, const void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes, \
    int n_ssrc, const int32_t* ssrc_key, const int32_t* ssrc_stream, const int32_t* payload_type, int payload_room, \
    int32_t* stream, int32_t* seq, int64_t* offsets, int32_t* num_bytes, int32_t* timestamp, uint8_t* marker, uint8_t* status, int32_t* stats
#define RTP_PARSE_ARGS \
    {n_items, ring, ring_capacity, dg_offsets, dg_sizes, n_ssrc, ssrc_key, ssrc_stream, payload_type, payload_room, \
     stream, seq, offsets, num_bytes, timestamp, marker, status, stats}
/* the checks every parse call makes first, in the header's order */
static LC3_Error rtp_parse_check(const rtp_parse_args* a)
{
    if (!a->ring || !a->dg_offsets || !a->dg_sizes || !a->ssrc_key || !a->ssrc_stream || !a->stream || !a->seq || !a->offsets || !a->num_bytes) return LC3_NULL_ERROR;
    if (a->n_items <= 0 || a->n_items >= LC3R_MAX_ITEMS || a->ring_capacity < 0 || a->n_ssrc <= 0 || a->payload_room < 0 || a->payload_room > LC3R_MAX_PAYLOAD_ROOM)
        return LC3_ERROR;
    return LC3_OK;
}
/* the rule on the host: the kernels' steps (lc3_rtp.inc) on the text they run */
LC3_Error lc3plus_plan_rtp_parse(int n_streams, RTP_PARSE_PARAMS, void* hip_stream, int sync)
{
    const rtp_parse_args a = RTP_PARSE_ARGS;
    const LC3_Error e = rtp_parse_check(&a);
    if (e) return e;
    if (n_streams <= 0) return LC3_ERROR;
    const lc3r_items out = {stream, seq, (long long*)offsets, num_bytes, timestamp, marker, status};
    if (stats) memset(stats, 0, sizeof(int32_t) * LC3R_STATS_WORDS);
    for (int64_t i = 0; i < n_items; i++) {
        const lc3r_item it = lc3r_parse((const uint8_t*)ring, ring_capacity, dg_offsets[i], dg_sizes[i], ssrc_key, ssrc_stream, n_ssrc, n_streams, payload_type,
                                        payload_room);
        lc3r_item_out(&out, i, &it);
        if (stats) stats[it.status]++;
    }
    return LC3_OK;
}
/* the SSRC table in the order the search needs: keys ascending as uint32, each with its stream (an insertion sort: tables are built once and are short) */
LC3_Error lc3plus_rtp_sort_ssrc(int n, int32_t* ssrc_key, int32_t* ssrc_stream)
{
    if (!ssrc_key || !ssrc_stream) return LC3_NULL_ERROR;
    if (n <= 0) return LC3_ERROR;
    for (int i = 1; i < n; i++) {
        const int32_t k = ssrc_key[i], v = ssrc_stream[i];
        int j = i;
        for (; j > 0 && (uint32_t)ssrc_key[j - 1] > (uint32_t)k; j--) { ssrc_key[j] = ssrc_key[j - 1]; ssrc_stream[j] = ssrc_stream[j - 1]; }
        ssrc_key[j] = k; ssrc_stream[j] = v;
    }
    for (int i = 1; i < n; i++) if (ssrc_key[i] == ssrc_key[i - 1]) return LC3_ERROR;
    return LC3_OK;
}
/* what a stamp call takes behind its batch, in the header's order */
typedef struct {
    int64_t max_packets; const int64_t* n_packets;
    const int32_t* pkt_route; const int32_t* pkt_seq; const int32_t* pkt_frame; const int64_t* pkt_offset; const int32_t* pkt_size; const uint8_t* pkt_flags;
    int n_routes; int n_frames; const int32_t* ssrc; const int32_t* ts_base; const int32_t* payload_type; int ts_step;
    int marker_mode; const uint8_t* cell_status; const uint8_t* resume; const int32_t* route_stats;
    void* wire; int64_t wire_capacity; int header_room; int payload_room;
    uint8_t* pkt_status; int32_t* next_ts; uint8_t* next_resume;
} rtp_stamp_args;
#define RTP_STAMP_PARAMS \
    int64_t max_packets, const int64_t* n_packets, \
    const int32_t* pkt_route, const int32_t* pkt_seq, const int32_t* pkt_frame, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_flags, \
    int n_routes, int n_frames, const int32_t* ssrc, const int32_t* ts_base, const int32_t* payload_type, int ts_step, \
    int marker_mode, const uint8_t* cell_status, const uint8_t* resume, const int32_t* route_stats, \
    void* wire, int64_t wire_capacity, int header_room, int payload_room, \
    uint8_t* pkt_status, int32_t* next_ts, uint8_t* next_resume
#define RTP_STAMP_ARGS \
    {max_packets, n_packets, pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, pkt_flags, n_routes, n_frames, ssrc, ts_base, payload_type, \
     ts_step, marker_mode, cell_status, resume, route_stats, wire, wire_capacity, header_room, payload_room, pkt_status, next_ts, next_resume}
/* the checks every stamp call makes first, in the header's order */
static LC3_Error rtp_stamp_check(const rtp_stamp_args* a)
{
    if (!a->n_packets || !a->pkt_route || !a->pkt_seq || !a->pkt_frame || !a->pkt_offset || !a->pkt_size || !a->ssrc || !a->ts_base || !a->payload_type || !a->wire)
        return LC3_NULL_ERROR;
    if (a->max_packets <= 0 || a->n_routes <= 0 || a->n_frames <= 0 || a->wire_capacity < 0 || a->payload_room < 0 || a->header_room < LC3R_FIXED ||
        a->header_room - LC3R_FIXED < a->payload_room)
        return LC3_ERROR;
    if (a->marker_mode != LC3R_MARKER_NEVER && a->marker_mode != LC3R_MARKER_AFTER_HOLE) return LC3_ERROR;
    if ((a->marker_mode == LC3R_MARKER_AFTER_HOLE || a->next_resume) && !a->cell_status) return LC3_ERROR;
    return LC3_OK;
}
static lc3r_stamp_in rtp_stamp_in(const rtp_stamp_args* a)
{
    const lc3r_stamp_in q = {a->pkt_route, a->pkt_seq, a->pkt_frame, (const long long*)a->pkt_offset, a->pkt_size, a->pkt_flags, a->ssrc, a->ts_base, a->payload_type,
                             a->cell_status, a->resume, a->route_stats, a->n_routes, a->n_frames, a->ts_step, a->marker_mode, a->header_room, a->payload_room,
                             (long long)a->wire_capacity};
    return q;
}
LC3_Error lc3plus_plan_rtp_stamp(RTP_STAMP_PARAMS, void* hip_stream, int sync)
{
    const rtp_stamp_args a = RTP_STAMP_ARGS;
    const LC3_Error e = rtp_stamp_check(&a);
    if (e) return e;
    const lc3r_stamp_in q = rtp_stamp_in(&a);
    const int64_t n = *n_packets < max_packets ? *n_packets : max_packets;
    for (int64_t p = 0; p < n; p++) {
        uint32_t hdr[3];
        long long at = 0;
        const int st = lc3r_stamp(&q, p, hdr, &at);
        if (st == LC3R_STAMPED) lc3r_header_out((uint8_t*)wire, at, hdr);
        if (pkt_status) pkt_status[p] = (uint8_t)st;
    }
    if (next_ts || next_resume)
        for (int r = 0; r < n_routes; r++) lc3r_route_out(&q, r, next_ts, next_resume);
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_rtp_parse(lc3plus_dec_batch* b, RTP_PARSE_PARAMS, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    const rtp_parse_args a = RTP_PARSE_ARGS;
    const LC3_Error e = rtp_parse_check(&a);
    if (e) return e;
    const lc3host_view v = lc3host_dec_view(b);
    lc3rtp_parse_call q;
    memset(&q, 0, sizeof q);
    q.n_streams = v.n_streams; q.n_ssrc = n_ssrc; q.payload_room = payload_room; q.sync = sync; q.n_items = (long long)n_items; q.ring_capacity = (long long)ring_capacity;
    q.ring = ring; q.dg_offsets = (const long long*)dg_offsets; q.dg_sizes = dg_sizes; q.ssrc_key = ssrc_key; q.ssrc_stream = ssrc_stream; q.payload_type = payload_type;
    q.out.stream = stream; q.out.seq = seq; q.out.offsets = (long long*)offsets; q.out.num_bytes = num_bytes; q.out.timestamp = timestamp; q.out.marker = marker;
    q.out.status = status; q.stats = stats;
    return SIBLING_RUN(lc3rtp_parse_call, SIB_RTP, 0, v, hip_stream, &q);
}
/* both stamp entry points end here: the checks, then the sibling */
static LC3_Error rtp_stamp_queue(lc3host_view v, const rtp_stamp_args* a, void* hip_stream, int sync)
{
    const LC3_Error e = rtp_stamp_check(a);
    if (e) return e;
    lc3rtp_stamp_call q;
    memset(&q, 0, sizeof q);
    q.sync = sync; q.max_packets = (long long)a->max_packets; q.n_packets = (const long long*)a->n_packets; q.in = rtp_stamp_in(a);
    q.wire = a->wire; q.pkt_status = a->pkt_status; q.next_ts = a->next_ts; q.next_resume = a->next_resume;
    return SIBLING_RUN(lc3rtp_stamp_call, SIB_RTP, 1, v, hip_stream, &q);
}
BATCH_TWINS(rtp_stamp, RTP_STAMP_PARAMS, rtp_stamp_args, RTP_STAMP_ARGS, rtp_stamp_queue(v, &a, hip_stream, sync))
/* ---- redundant audio (include/lc3plus_batch.h "Redundant audio"; lc3_red_shim.h) ---- */
/* what every pack call takes behind its batch, in the header's order */
typedef struct {
    int n_frames; const void* frames; int64_t frames_capacity; const int64_t* offsets; const int32_t* num_bytes; int max_frame_bytes;
    const uint8_t* flags; int skip_mask; const int32_t* counts; int n_routes; const int32_t* route_src;
    int64_t max_packets; const int64_t* n_packets; const int32_t* pkt_route; const int32_t* pkt_frame;
    int max_depth; const int32_t* depth; const int32_t* block_pt; int ts_step; int max_packet_bytes;
    const uint8_t* tail_bytes_in; const int32_t* tail_sizes_in; int tail_stride; uint8_t* tail_bytes_out; int32_t* tail_sizes_out;
    void* wire; int64_t wire_capacity; int header_room; int align;
    int64_t* red_offset; int32_t* red_size; uint8_t* red_flags; uint8_t* red_blocks; int64_t* wire_total; int32_t* route_stats;
    void* work;
} red_pack_args;
#define RED_PACK_PARAMS \
    int n_frames, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes, int max_frame_bytes, \
    const uint8_t* flags, int skip_mask, const int32_t* counts, int n_routes, const int32_t* route_src, \
    int64_t max_packets, const int64_t* n_packets, const int32_t* pkt_route, const int32_t* pkt_frame, \
    int max_depth, const int32_t* depth, const int32_t* block_pt, int ts_step, int max_packet_bytes, \
    const uint8_t* tail_bytes_in, const int32_t* tail_sizes_in, int tail_stride, uint8_t* tail_bytes_out, int32_t* tail_sizes_out, \
    void* wire, int64_t wire_capacity, int header_room, int align, \
    int64_t* red_offset, int32_t* red_size, uint8_t* red_flags, uint8_t* red_blocks, int64_t* wire_total, int32_t* route_stats, \
    void* work
#define RED_PACK_ARGS \
    {n_frames, frames, frames_capacity, offsets, num_bytes, max_frame_bytes, flags, skip_mask, counts, n_routes, route_src, max_packets, n_packets, \
     pkt_route, pkt_frame, max_depth, depth, block_pt, ts_step, max_packet_bytes, tail_bytes_in, tail_sizes_in, tail_stride, tail_bytes_out, \
     tail_sizes_out, wire, wire_capacity, header_room, align, red_offset, red_size, red_flags, red_blocks, wire_total, route_stats, work}
/* the checks every pack call makes first, in the header's order; n_streams < 0: not known yet (the batch is looked at behind them) */
static LC3_Error red_pack_check(const red_pack_args* a, int n_streams)
{
    if (!a->frames || !a->offsets || !a->num_bytes || !a->n_packets || !a->pkt_route || !a->pkt_frame || !a->block_pt || !a->wire || !a->red_offset || !a->red_size ||
        !a->work)
        return LC3_NULL_ERROR;
    if (a->n_frames <= 0 || a->n_routes <= 0 || a->max_frame_bytes <= 0 || a->frames_capacity < 0 || a->wire_capacity < 0 || a->max_packets <= 0 ||
        a->max_packets >= LC3RED_MAX_PACKETS)
        return LC3_ERROR;
    if (a->max_depth < 0 || a->max_depth > LC3RED_MAX_DEPTH || a->ts_step <= 0 || a->max_packet_bytes < 0) return LC3_ERROR;
    if (!a->tail_bytes_in != !a->tail_sizes_in || !a->tail_bytes_out != !a->tail_sizes_out) return LC3_ERROR;
    if (a->max_depth && (a->tail_sizes_in || a->tail_sizes_out) && ((a->tail_stride & 15) || a->tail_stride < IMIN(a->max_frame_bytes, LC3RED_MAX_BLOCK))) return LC3_ERROR;
    if (a->header_room < 0 || a->header_room > INT32_MAX - LC3E_MAX_ALIGN - LC3RED_MAX_EXTRA - a->max_frame_bytes) return LC3_ERROR;
    if (a->align < 1 || a->align > LC3E_MAX_ALIGN || (a->align & (a->align - 1))) return LC3_ERROR;
    if (n_streams >= 0 && !a->route_src && a->n_routes != n_streams) return LC3_ERROR;
    if ((uintptr_t)a->work & 7) return LC3_ERROR;
    return LC3_OK;
}
static lc3red_pack_in red_pack_in(const red_pack_args* a, int n_streams)
{
    const lc3red_pack_in q = {a->frames, (const long long*)a->offsets, a->num_bytes, a->flags, a->counts, a->route_src, a->pkt_route, a->pkt_frame, a->depth, a->block_pt,
                              a->tail_bytes_in, a->tail_sizes_in, (long long)a->frames_capacity, (long long)a->wire_capacity, n_streams, a->n_frames, a->max_frame_bytes,
                              a->skip_mask, a->n_routes, a->max_depth, a->ts_step, a->max_packet_bytes, a->tail_stride, a->header_room, a->align};
    return q;
}
int64_t lc3plus_red_work_bytes(int64_t max_packets)
{
    if (max_packets <= 0 || max_packets >= LC3RED_MAX_PACKETS) return 0;
    return lc3red_work_bytes((long long)max_packets);
}
/* the rule on the host: the steps of the kernels (lc3_red.inc) one after the other, on the text they run and over the same workspace */
LC3_Error lc3plus_plan_red_pack(int n_streams, RED_PACK_PARAMS, void* hip_stream, int sync)
{
    const red_pack_args a = RED_PACK_ARGS;
    LC3_Error e = red_pack_check(&a, -1);
    if (e) return e;
    if (n_streams <= 0) return LC3_ERROR;
    e = red_pack_check(&a, n_streams);
    if (e) return e;
    const lc3red_pack_in q = red_pack_in(&a, n_streams);
    const long long n = lc3red_count((const long long*)n_packets, max_packets), n_tiles = lc3red_tiles(max_packets);
    int32_t* size = (int32_t*)work;
    long long* sums = (long long*)((char*)work + lc3red_work_sums(max_packets));
    uint8_t* mask = (uint8_t*)work + lc3red_work_mask(max_packets);
    /* size */
    if (route_stats) memset(route_stats, 0, sizeof(int32_t) * LC3RED_RS_WORDS * (size_t)n_routes);
    for (long long p = 0; p < n; p++) {
        int s = 0, m = 0;
        size[p] = lc3red_packet(&q, pkt_route[p], pkt_frame[p], &s, &m);
        mask[p] = (uint8_t)m;
    }
    /* the tiles' sums, then their bases and the total */
    for (long long b = 0; b < n_tiles; b++) {
        long long bytes = 0;
        for (long long p = b * LC3RED_TILE; p < n && p < (b + 1) * LC3RED_TILE; p++) bytes += lc3red_advance(size[p], align);
        sums[b] = bytes;
    }
    long long run_b = 0;
    for (long long b = 0; b < n_tiles; b++) { const long long bytes = sums[b]; sums[b] = run_b; run_b += bytes; }
    if (wire_total) *wire_total = run_b;
    /* scatter, and the copy of each packet that fits */
    for (long long b = 0; b < n_tiles; b++) {
        long long run = sums[b];
        for (long long p = b * LC3RED_TILE; p < n && p < (b + 1) * LC3RED_TILE; p++) {
            const int32_t sz = size[p];
            const int fit = lc3e_fits(run, sz, 1, wire_capacity);
            red_offset[p] = run; red_size[p] = sz;
            if (red_flags) red_flags[p] = (uint8_t)(sz <= 0 ? LC3RED_PKT_BAD : fit ? 0 : LC3E_PKT_OVERFLOW);
            if (red_blocks) red_blocks[p] = (uint8_t)(mask[p] & 15);
            if (sz > 0) {
                const int r = pkt_route[p], t = pkt_frame[p], s = route_src ? route_src[r] : r, m = mask[p] & 15;
                int k = 0, block_bytes = 0;
                for (int j = 1; j <= max_depth; j++) k += m >> (j - 1) & 1;
                uint8_t* hdr = (uint8_t*)wire + run + header_room;
                uint8_t* body = hdr + 4 * k + 1;
                uintptr_t src = 0;
                for (int j = max_depth; j >= 1; j--) {
                    if (!(m >> (j - 1) & 1)) continue;
                    const int32_t bs = lc3red_block(&q, s, t - j, &src);
                    block_bytes += bs;
                    if (!fit) continue;
                    const uint32_t h = lc3red_header(block_pt[r], j * ts_step, bs);
                    for (int l = 0; l < 4; l++) hdr[l] = (uint8_t)(h >> (8 * l));
                    egress_copy(body, (const uint8_t*)src, bs);
                    hdr += 4; body += bs;
                }
                if (fit) {
                    const int32_t nb = lc3red_block(&q, s, t, &src);
                    *hdr = (uint8_t)(block_pt[r] & 127);
                    egress_copy(body, (const uint8_t*)src, nb);
                }
                if (route_stats) {
                    int32_t* st = route_stats + (size_t)r * LC3RED_RS_WORDS;
                    st[LC3RED_RS_PACKETS]++; st[LC3RED_RS_BLOCKS] += k; st[LC3RED_RS_BLOCK_BYTES] += block_bytes; st[LC3RED_RS_MISSED] += mask[p] >> 4;
                }
            }
            run += lc3red_advance(sz, align);
        }
    }
    /* the tails */
    if (tail_sizes_out)
        for (int s = 0; s < n_streams; s++)
            for (int g = 0; g < max_depth; g++) {
                uintptr_t src = 0;
                const size_t e_ = (size_t)s * max_depth + g;
                const int32_t nb = lc3red_tail(&q, s, g, &src);
                tail_sizes_out[e_] = nb;
                if (nb > 0) egress_copy(tail_bytes_out + e_ * (size_t)tail_stride, (const uint8_t*)src, nb);
            }
    return LC3_OK;
}
/* both pack entry points end here: the checks, the one that needs the batch's n_streams behind the others, then the sibling */
static LC3_Error red_pack_queue(lc3host_view v, const red_pack_args* a, void* hip_stream, int sync)
{
    const LC3_Error e = red_pack_check(a, -1);
    if (e) return e;
    if (!a->route_src && a->n_routes != v.n_streams) return LC3_ERROR;
    lc3red_pack_call q;
    memset(&q, 0, sizeof q);
    q.sync = sync; q.max_packets = (long long)a->max_packets; q.n_packets = (const long long*)a->n_packets; q.in = red_pack_in(a, v.n_streams);
    q.tail_bytes_out = a->tail_bytes_out; q.tail_sizes_out = a->tail_sizes_out; q.wire = a->wire;
    q.red_offset = (long long*)a->red_offset; q.red_size = a->red_size; q.red_flags = a->red_flags; q.red_blocks = a->red_blocks; q.wire_total = (long long*)a->wire_total;
    q.route_stats = a->route_stats; q.work = a->work;
    return SIBLING_RUN(lc3red_pack_call, SIB_RED, 0, v, hip_stream, &q);
}
BATCH_TWINS(red_pack, RED_PACK_PARAMS, red_pack_args, RED_PACK_ARGS, red_pack_queue(v, &a, hip_stream, sync))
/* what an unpack call takes behind its batch, in the header's order */
typedef struct {
    int64_t n_items; const int32_t* stream; const int32_t* seq; const int64_t* offsets; const int32_t* num_bytes; const int32_t* timestamp;
    const void* ring; int64_t ring_capacity; int max_red; const int32_t* block_pt; int ts_step;
    int32_t* out_stream; int32_t* out_seq; int64_t* out_offsets; int32_t* out_num_bytes; int32_t* out_timestamp; uint8_t* out_gen; uint8_t* status; int32_t* stats;
} red_unpack_args;
#define RED_UNPACK_PARAMS \
    int64_t n_items, const int32_t* stream, const int32_t* seq, const int64_t* offsets, const int32_t* num_bytes, const int32_t* timestamp, \
    const void* ring, int64_t ring_capacity, int max_red, const int32_t* block_pt, int ts_step, \
    int32_t* out_stream, int32_t* out_seq, int64_t* out_offsets, int32_t* out_num_bytes, int32_t* out_timestamp, uint8_t* out_gen, uint8_t* status, int32_t* stats
#define RED_UNPACK_ARGS \
    {n_items, stream, seq, offsets, num_bytes, timestamp, ring, ring_capacity, max_red, block_pt, ts_step, \
     out_stream, out_seq, out_offsets, out_num_bytes, out_timestamp, out_gen, status, stats}
static LC3_Error red_unpack_check(const red_unpack_args* a)
{
    if (!a->stream || !a->seq || !a->offsets || !a->num_bytes || !a->ring || !a->out_stream || !a->out_seq || !a->out_offsets || !a->out_num_bytes) return LC3_NULL_ERROR;
    if (a->n_items <= 0 || a->n_items >= LC3R_MAX_ITEMS || a->ring_capacity < 0 || a->max_red < 0 || a->max_red > LC3RED_MAX_DEPTH || a->ts_step <= 0) return LC3_ERROR;
    return LC3_OK;
}
static lc3red_unpack_io red_unpack_io(const red_unpack_args* a, int n_streams)
{
    const lc3red_unpack_io q = {a->stream, a->seq, (const long long*)a->offsets, a->num_bytes, a->timestamp, (const uint8_t*)a->ring, a->block_pt, a->out_stream, a->out_seq,
                                (long long*)a->out_offsets, a->out_num_bytes, a->out_timestamp, a->out_gen, a->status, (long long)a->ring_capacity, n_streams, a->max_red,
                                a->ts_step};
    return q;
}
/* the rule on the host: the kernels' steps (lc3_red.inc) on the text they run */
LC3_Error lc3plus_plan_red_unpack(int n_streams, RED_UNPACK_PARAMS, void* hip_stream, int sync)
{
    const red_unpack_args a = RED_UNPACK_ARGS;
    const LC3_Error e = red_unpack_check(&a);
    if (e) return e;
    if (n_streams <= 0) return LC3_ERROR;
    const lc3red_unpack_io q = red_unpack_io(&a, n_streams);
    if (stats) memset(stats, 0, sizeof(int32_t) * LC3RED_STATS_WORDS);
    for (int64_t i = 0; i < n_items; i++) {
        int drops[3] = {0, 0, 0};
        const int st = lc3red_unpack(&q, i, drops);
        if (stats) { stats[st]++; stats[LC3RED_ST_DROP_TYPE] += drops[0]; stats[LC3RED_ST_DROP_OFFSET] += drops[1]; stats[LC3RED_ST_DROP_EMPTY] += drops[2]; }
    }
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_red_unpack(lc3plus_dec_batch* b, RED_UNPACK_PARAMS, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    const red_unpack_args a = RED_UNPACK_ARGS;
    const LC3_Error e = red_unpack_check(&a);
    if (e) return e;
    const lc3host_view v = lc3host_dec_view(b);
    lc3red_unpack_call q;
    memset(&q, 0, sizeof q);
    q.sync = sync; q.n_items = (long long)n_items; q.io = red_unpack_io(&a, v.n_streams); q.stats = stats;
    return SIBLING_RUN(lc3red_unpack_call, SIB_RED, 1, v, hip_stream, &q);
}
/* ---- generic FEC (include/lc3plus_batch.h "Generic FEC"; lc3_fec_shim.h) ---- */
/* what every encode call takes behind its batch, in the header's order */
typedef struct {
    int64_t max_packets; const int64_t* n_packets; const int32_t* pkt_route; const int32_t* pkt_frame; const int64_t* pkt_offset; const int32_t* pkt_size;
    const uint8_t* pkt_status; const void* wire; int64_t wire_capacity; int header_room; int payload_room;
    int n_routes; int n_frames; const int32_t* seq_base; const int32_t* route_stats; const int32_t* group; const uint8_t* flush; const int32_t* fec_seq_base;
    const int32_t* state_in; const uint8_t* acc_in; int32_t* state_out; uint8_t* acc_out; int acc_stride;
    void* fec_wire; int64_t fec_capacity; int64_t fec_stride; int fec_header_room;
    int64_t max_fec_packets; int64_t* n_fec; int32_t* fec_route; int32_t* fec_seq; int32_t* fec_frame; int64_t* fec_offset; int32_t* fec_size; uint8_t* fec_flags;
    int32_t* fec_mask; int32_t* next_fec_seq; int32_t* route_stats_out; void* work;
} fec_encode_args;
/* the checks every encode call makes first, in the header's order */
static LC3_Error fec_encode_check(const fec_encode_args* a)
{
    if (!a->n_packets || !a->pkt_route || !a->pkt_frame || !a->pkt_offset || !a->pkt_size || !a->wire || !a->seq_base || !a->group || !a->fec_seq_base || !a->fec_wire ||
        !a->n_fec || !a->fec_route || !a->fec_seq || !a->fec_frame || !a->fec_offset || !a->fec_size || !a->work)
        return LC3_NULL_ERROR;
    if (a->max_packets <= 0 || a->max_packets >= LC3FEC_MAX_PACKETS || a->wire_capacity < 0 || a->payload_room < 0 || a->header_room < LC3R_FIXED + a->payload_room)
        return LC3_ERROR;
    if (a->n_routes <= 0 || a->n_frames <= 0 || (long long)a->n_routes * a->n_frames >= LC3E_MAX_CELLS) return LC3_ERROR;
    const int given = (a->state_in != NULL) + (a->acc_in != NULL) + (a->state_out != NULL) + (a->acc_out != NULL);
    if (given != 0 && given != 4) return LC3_ERROR;
    if (given && (a->acc_stride <= 0 || (a->acc_stride & 15))) return LC3_ERROR;
    if (given) {                                                      /* an out buffer may not meet its in buffer: the rows of different routes are different waves */
        const uintptr_t sb = sizeof(int32_t) * LC3FEC_STATE_WORDS * (uintptr_t)a->n_routes, ab = (uintptr_t)a->acc_stride * (uintptr_t)a->n_routes;
        const uintptr_t si = (uintptr_t)a->state_in, so = (uintptr_t)a->state_out, ai = (uintptr_t)a->acc_in, ao = (uintptr_t)a->acc_out;
        if ((si < so + sb && so < si + sb) || (ai < ao + ab && ao < ai + ab)) return LC3_ERROR;
    }
    if (a->fec_capacity < 0 || a->fec_stride <= 0 || a->fec_stride > LC3FEC_MAX_STRIDE || a->fec_header_room < LC3R_FIXED || a->fec_header_room > LC3FEC_MAX_PKT ||
        a->max_fec_packets <= 0)
        return LC3_ERROR;
    const uintptr_t w0 = (uintptr_t)a->wire, d0 = (uintptr_t)a->fec_wire;
    if (d0 < w0 + (uintptr_t)a->wire_capacity && w0 < d0 + (uintptr_t)a->fec_capacity) return LC3_ERROR;              /* out of place only */
    if ((uintptr_t)a->work & 7) return LC3_ERROR;
    return LC3_OK;
}
static void fec_encode_io(const fec_encode_args* a, lc3fec_enc_in* q, lc3fec_enc_out* o)
{
    const lc3fec_enc_in in = {(const long long*)a->n_packets, a->pkt_route, a->pkt_frame, (const long long*)a->pkt_offset, a->pkt_size, a->pkt_status,
                              (const uint8_t*)a->wire, a->seq_base, a->route_stats, a->group, a->flush, a->fec_seq_base, a->state_in, a->acc_in,
                              (long long)a->max_packets, (long long)a->wire_capacity, (long long)a->max_fec_packets, (long long)a->fec_capacity, (long long)a->fec_stride,
                              a->header_room, a->payload_room, a->n_routes, a->n_frames, a->state_in ? a->acc_stride : 0, a->fec_header_room, a->state_out != NULL};
    const lc3fec_enc_out out = {(long long*)a->n_fec, a->fec_route, a->fec_seq, a->fec_frame, (long long*)a->fec_offset, a->fec_size, a->fec_flags, a->fec_mask,
                                a->next_fec_seq, a->route_stats_out, a->state_out, a->acc_out, (uint8_t*)a->fec_wire};
    *q = in; *o = out;
}
int64_t lc3plus_fec_work_bytes(int n_routes, int n_frames)
{
    if (n_routes <= 0 || n_frames <= 0 || (long long)n_routes * n_frames >= LC3E_MAX_CELLS) return 0;
    return lc3fec_work_bytes(n_routes, n_frames);
}
int64_t lc3plus_fec_recover_work_bytes(int n_streams, int window)
{
    if (n_streams <= 0 || window < 64 || window > 65536 || (window & (window - 1))) return 0;
    return lc3fec_recover_work_bytes(n_streams, window);
}
/* dst[0 .. n) ^= src[0 .. n) */
static void fec_xor(uint8_t* dst, const uint8_t* src, int n) { for (int i = 0; i < n; i++) dst[i] ^= src[i]; }
#define FEC_ENCODE_PARAMS \
    int64_t max_packets, const int64_t* n_packets, const int32_t* pkt_route, const int32_t* pkt_frame, const int64_t* pkt_offset, const int32_t* pkt_size, \
    const uint8_t* pkt_status, const void* wire, int64_t wire_capacity, int header_room, int payload_room, \
    int n_routes, int n_frames, const int32_t* seq_base, const int32_t* route_stats, const int32_t* group, const uint8_t* flush, const int32_t* fec_seq_base, \
    const int32_t* state_in, const uint8_t* acc_in, int32_t* state_out, uint8_t* acc_out, int acc_stride, \
    void* fec_wire, int64_t fec_capacity, int64_t fec_stride, int fec_header_room, \
    int64_t max_fec_packets, int64_t* n_fec, int32_t* fec_route, int32_t* fec_seq, int32_t* fec_frame, int64_t* fec_offset, int32_t* fec_size, uint8_t* fec_flags, \
    int32_t* fec_mask, int32_t* next_fec_seq, int32_t* route_stats_out, void* work
#define FEC_ENCODE_ARGS \
    {max_packets, n_packets, pkt_route, pkt_frame, pkt_offset, pkt_size, pkt_status, wire, wire_capacity, header_room, payload_room, n_routes, n_frames, seq_base, \
     route_stats, group, flush, fec_seq_base, state_in, acc_in, state_out, acc_out, acc_stride, fec_wire, fec_capacity, fec_stride, fec_header_room, max_fec_packets, \
     n_fec, fec_route, fec_seq, fec_frame, fec_offset, fec_size, fec_flags, fec_mask, next_fec_seq, route_stats_out, work}
/* the rule on the host: the steps of the kernels (lc3_fec.inc) one after the other, on the text they run and over the same workspace */
LC3_Error lc3plus_plan_fec_encode(FEC_ENCODE_PARAMS, void* hip_stream, int sync)
{
    (void)hip_stream; (void)sync;
    const fec_encode_args a = FEC_ENCODE_ARGS;
    const LC3_Error e = fec_encode_check(&a);
    if (e) return e;
    lc3fec_enc_in q;
    lc3fec_enc_out o;
    fec_encode_io(&a, &q, &o);
    const long long cells = (long long)n_routes * n_frames, n = lc3fec_count(q.n_packets, q.max_packets), n_tiles = lc3fec_tiles(n_routes);
    int32_t* map = (int32_t*)work;
    long long* sums = (long long*)((char*)work + lc3fec_work_sums(n_routes, n_frames));
    long long* qbase = (long long*)((char*)work + lc3fec_work_qbase(n_routes, n_frames));
    int32_t* fseq = (int32_t*)((char*)work + lc3fec_work_fseq(n_routes, n_frames));
    /* fill and scatter */
    for (long long i = 0; i < cells; i++) map[i] = LC3FEC_NO_ENTRY;
    for (long long p = 0; p < n; p++) {
        const long long cell = lc3fec_entry_cell(&q, p);
        if (cell >= 0 && (int32_t)p < map[cell]) map[cell] = (int32_t)p;
    }
    /* the tiles' sums, their bases and the total, then every route's first entry */
    for (long long b = 0; b < n_tiles; b++) {
        long long s = 0;
        for (long long r = b * LC3FEC_TILE; r < n_routes && r < (b + 1) * LC3FEC_TILE; r++) s += lc3fec_route_plan(&q, (int)r).nclosed;
        sums[b] = s;
    }
    long long run_b = 0;
    for (long long b = 0; b < n_tiles; b++) { const long long s = sums[b]; sums[b] = run_b; run_b += s; }
    *n_fec = run_b;
    for (long long b = 0; b < n_tiles; b++) {
        long long run = sums[b];
        for (long long r = b * LC3FEC_TILE; r < n_routes && r < (b + 1) * LC3FEC_TILE; r++) {
            const int w = lc3fec_route_plan(&q, (int)r).nclosed;
            qbase[r] = run;
            fseq[r] = fec_seq_base[r];                                /* next_fec_seq may be fec_seq_base: the records are numbered from this copy */
            if (next_fec_seq) next_fec_seq[r] = (int32_t)((uint32_t)fseq[r] + (uint32_t)w);
            if (route_stats_out) memset(route_stats_out + r * LC3FEC_RS_WORDS, 0, sizeof(int32_t) * LC3FEC_RS_WORDS);
            run += w;
        }
    }
    /* the groups */
    for (int r = 0; r < n_routes; r++) {
        const lc3fec_plan P = lc3fec_route_plan(&q, r);
        for (int g = 0; g < P.ng; g++) {
            const lc3fec_group G = lc3fec_group_of(&P, g);
            long long at[LC3FEC_MAX_GROUP];
            int32_t len[LC3FEC_MAX_GROUP];
            const int cnt = G.t1 - G.t0;
            for (int i = 0; i < cnt; i++) { at[i] = 0; len[i] = -1; if (!lc3fec_member(&q, map, r, G.t0 + i, &at[i], &len[i])) len[i] = -1; }
            const lc3fec_fold f = lc3fec_fold_group(&q, r, &G, at, len);
            uint8_t* dst = NULL;
            int nbytes = 0;
            if (G.closes) {
                const long long en = qbase[r] + g;
                int32_t size = 0;
                if (route_stats_out) route_stats_out[(size_t)r * LC3FEC_RS_WORDS + LC3FEC_RS_GROUPS]++;
                if (!lc3fec_emit(&q, &o, r, g, &G, &f, en, fseq[r], &size)) continue;
                uint32_t w[4];
                dst = o.fec_wire + en * q.fec_stride + q.fec_header_room;
                lc3fec_header(&f, w);
                lc3fec_header_out(dst, w);
                dst += LC3FEC_HEADER; nbytes = f.plen;
                if (route_stats_out) {
                    int32_t* st = route_stats_out + (size_t)r * LC3FEC_RS_WORDS;
                    st[LC3FEC_RS_PACKETS]++; st[LC3FEC_RS_MEDIA] += __builtin_popcount(f.mask); st[LC3FEC_RS_BYTES] += f.plen;
                }
                memset(dst, 0, (size_t)nbytes);
            } else if (q.carry) {
                const int keep = lc3fec_state_out(&q, state_out + (size_t)r * LC3FEC_STATE_WORDS, &G, &f);
                dst = acc_out + (size_t)r * acc_stride;
                memset(dst, 0, (size_t)acc_stride);
                if (!keep) continue;
            } else continue;
            if (G.F0 > 0) {                                           /* the carried accumulator counts up to the length the state names */
                int32_t xlen = state_in[(size_t)r * LC3FEC_STATE_WORDS + LC3FEC_S_MAX];
                xlen = xlen < 0 || xlen > q.acc_stride || xlen > f.plen ? 0 : xlen;
                fec_xor(dst, acc_in + (size_t)r * acc_stride, xlen);
            }
            for (int i = 0; i < cnt; i++)
                if (len[i] > 0) fec_xor(dst, q.wire + at[i], len[i]);
        }
        if (q.carry && !P.open) {                                     /* no open group: the state is handed through (c = 0) or ends */
            if (P.c == 0) {
                memcpy(state_out + (size_t)r * LC3FEC_STATE_WORDS, state_in + (size_t)r * LC3FEC_STATE_WORDS, sizeof(int32_t) * LC3FEC_STATE_WORDS);
                memcpy(acc_out + (size_t)r * acc_stride, acc_in + (size_t)r * acc_stride, (size_t)acc_stride);
            } else {
                memset(state_out + (size_t)r * LC3FEC_STATE_WORDS, 0, sizeof(int32_t) * LC3FEC_STATE_WORDS);
                memset(acc_out + (size_t)r * acc_stride, 0, (size_t)acc_stride);
            }
        }
    }
    return LC3_OK;
}
/* both encode entry points end here: the checks, then the sibling */
static LC3_Error fec_encode_queue(lc3host_view v, const fec_encode_args* a, void* hip_stream, int sync)
{
    const LC3_Error e = fec_encode_check(a);
    if (e) return e;
    lc3fec_encode_call q;
    memset(&q, 0, sizeof q);
    q.sync = sync; q.work = a->work;
    fec_encode_io(a, &q.in, &q.out);
    return SIBLING_RUN(lc3fec_encode_call, SIB_FEC, 0, v, hip_stream, &q);
}
BATCH_TWINS(fec_encode, FEC_ENCODE_PARAMS, fec_encode_args, FEC_ENCODE_ARGS, fec_encode_queue(v, &a, hip_stream, sync))
/* what a recover call takes behind its batch, in the header's order */
typedef struct {
    int64_t n_items; void* ring; int64_t ring_capacity; const int64_t* dg_offsets; const int32_t* dg_sizes; const int32_t* stream; const int32_t* seq;
    int64_t n_fec; const int32_t* fec_stream; const int64_t* fec_offsets; const int32_t* fec_num_bytes; int window; const int32_t* ssrc;
    int64_t rec_offset; int64_t rec_stride; int64_t* rec_dg_offsets; int32_t* rec_dg_sizes; int32_t* rec_seq; uint8_t* status; int32_t* stats; void* work;
} fec_recover_args;
static LC3_Error fec_recover_check(const fec_recover_args* a)
{
    if (!a->ring || !a->dg_offsets || !a->dg_sizes || !a->stream || !a->seq || !a->fec_stream || !a->fec_offsets || !a->fec_num_bytes || !a->ssrc ||
        !a->rec_dg_offsets || !a->rec_dg_sizes || !a->rec_seq || !a->work)
        return LC3_NULL_ERROR;
    if (a->n_items <= 0 || a->n_items >= LC3R_MAX_ITEMS || a->ring_capacity < 0 || a->n_fec <= 0 || a->n_fec >= LC3R_MAX_ITEMS) return LC3_ERROR;
    if (a->window < 64 || a->window > 65536 || (a->window & (a->window - 1))) return LC3_ERROR;
    if (a->rec_offset < 0 || a->rec_stride < LC3R_FIXED || a->rec_stride > LC3FEC_MAX_STRIDE || ((uintptr_t)a->work & 7)) return LC3_ERROR;
    return LC3_OK;
}
static lc3fec_rec_io fec_recover_io(const fec_recover_args* a, int n_streams)
{
    const lc3fec_rec_io q = {(uint8_t*)a->ring, (const long long*)a->dg_offsets, a->dg_sizes, a->stream, a->seq, a->fec_stream, (const long long*)a->fec_offsets,
                             a->fec_num_bytes, a->ssrc, (long long*)a->rec_dg_offsets, a->rec_dg_sizes, a->rec_seq, a->status, (long long)a->ring_capacity,
                             (long long)a->n_items, (long long)a->n_fec, (long long)a->rec_offset, (long long)a->rec_stride, n_streams, a->window};
    return q;
}
#define FEC_RECOVER_PARAMS \
    int64_t n_items, void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes, const int32_t* stream, const int32_t* seq, \
    int64_t n_fec, const int32_t* fec_stream, const int64_t* fec_offsets, const int32_t* fec_num_bytes, int window, const int32_t* ssrc, \
    int64_t rec_offset, int64_t rec_stride, int64_t* rec_dg_offsets, int32_t* rec_dg_sizes, int32_t* rec_seq, uint8_t* status, int32_t* stats, void* work
#define FEC_RECOVER_ARGS \
    {n_items, ring, ring_capacity, dg_offsets, dg_sizes, stream, seq, n_fec, fec_stream, fec_offsets, fec_num_bytes, window, ssrc, rec_offset, rec_stride, \
     rec_dg_offsets, rec_dg_sizes, rec_seq, status, stats, work}
/* the rule on the host: the kernels' steps (lc3_fec.inc) on the text they run */
LC3_Error lc3plus_plan_fec_recover(int n_streams, FEC_RECOVER_PARAMS, void* hip_stream, int sync)
{
    (void)hip_stream; (void)sync;
    const fec_recover_args a = FEC_RECOVER_ARGS;
    const LC3_Error e = fec_recover_check(&a);
    if (e) return e;
    if (n_streams <= 0) return LC3_ERROR;
    const lc3fec_rec_io q = fec_recover_io(&a, n_streams);
    int32_t* table = (int32_t*)work;
    for (long long i = 0; i < (long long)n_streams * window; i++) table[i] = LC3FEC_NO_ENTRY;
    for (long long i = 0; i < n_items; i++) {
        const int s = stream[i];
        if (s < 0 || s >= n_streams) continue;
        int32_t* e_ = table + (size_t)s * window + ((uint32_t)seq[i] & (uint32_t)(window - 1));
        if ((int32_t)i < *e_) *e_ = (int32_t)i;
    }
    if (stats) memset(stats, 0, sizeof(int32_t) * LC3FEC_STATS_WORDS);
    for (long long f = 0; f < n_fec; f++) {
        const int st = lc3fec_verdict(&q, table, f);
        if (stats) stats[st]++;
        if (st != LC3FEC_RECOVERED) continue;
        lc3fec_item h;
        lc3fec_item_header(&q, f, &h);
        const int rl = rec_dg_sizes[f] - LC3R_FIXED;
        uint8_t* dst = q.ring + rec_dg_offsets[f] + LC3R_FIXED;
        memcpy(dst, q.ring + fec_offsets[f] + h.hl, (size_t)rl);
        for (int i = 0; i < (h.hl == LC3FEC_HEADER ? 16 : LC3FEC_MAX_BITS); i++) {
            long long at = 0;
            int32_t len = 0;
            if (!(h.mask >> (LC3FEC_MAX_BITS - 1 - i) & 1) || !lc3fec_lookup(&q, table, fec_stream[f], (h.sn + (uint32_t)i) & 0xFFFFu, &at, &len)) continue;
            fec_xor(dst, q.ring + at, IMIN(len, rl));
        }
    }
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_fec_recover(lc3plus_dec_batch* b, FEC_RECOVER_PARAMS, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    const fec_recover_args a = FEC_RECOVER_ARGS;
    const LC3_Error e = fec_recover_check(&a);
    if (e) return e;
    const lc3host_view v = lc3host_dec_view(b);
    lc3fec_recover_call q;
    memset(&q, 0, sizeof q);
    q.sync = sync; q.io = fec_recover_io(&a, v.n_streams); q.stats = stats; q.work = work;
    return SIBLING_RUN(lc3fec_recover_call, SIB_FEC, 1, v, hip_stream, &q);
}
/* ---- generic FEC, repair across calls (include/lc3plus_batch.h "Generic FEC", REPAIR; lc3_repair_shim.h) ---- */
/* what a repair call takes behind its batch, in the header's order */
typedef struct {
    int64_t n_items; void* ring; int64_t ring_capacity; const int64_t* dg_offsets; const int32_t* dg_sizes; const int32_t* stream; const int32_t* seq;
    int64_t n_fec; const int32_t* fec_stream; const int64_t* fec_offsets; const int32_t* fec_num_bytes; const int32_t* fec_seq; const int32_t* ssrc;
    int64_t med_offset; int med_slots; int med_stride; int32_t* med_seq; int32_t* med_size;
    void* fec_store; int fec_slots; int fec_stride; int32_t* cell_seq; int32_t* cell_size; uint8_t* cell_status; int32_t* state; int passes;
    int64_t* rec_dg_offsets; int32_t* rec_dg_sizes; int32_t* rec_seq; uint8_t* item_status; uint8_t* fec_status; int32_t* stats; void* work;
} fec_repair_args;
static int pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && !(v & (v - 1)); }
static LC3_Error fec_repair_check(const fec_repair_args* a, int n_streams)
{
    if (!a->ring || !a->ssrc || !a->med_seq || !a->med_size || !a->fec_store || !a->cell_seq || !a->cell_size || !a->cell_status || !a->state || !a->rec_dg_offsets ||
        !a->rec_dg_sizes || !a->rec_seq || !a->work)
        return LC3_NULL_ERROR;
    if (a->n_items > 0 && (!a->dg_offsets || !a->dg_sizes || !a->stream || !a->seq)) return LC3_NULL_ERROR;
    if (a->n_fec > 0 && (!a->fec_stream || !a->fec_offsets || !a->fec_num_bytes || !a->fec_seq)) return LC3_NULL_ERROR;
    if (n_streams <= 0 || a->n_items < 0 || a->n_items >= LC3R_MAX_ITEMS || a->ring_capacity < 0 || a->n_fec < 0 || a->n_fec >= LC3R_MAX_ITEMS) return LC3_ERROR;
    if (a->med_offset < 0 || (a->med_offset & 15) || !pow2_in(a->med_slots, LC3REP_MIN_MED, LC3REP_MAX_MED) || a->med_stride < 16 || a->med_stride > LC3FEC_MAX_PKT ||
        (a->med_stride & 15))
        return LC3_ERROR;
    if (!pow2_in(a->fec_slots, LC3REP_MIN_CELLS, LC3REP_MAX_CELLS) || a->fec_stride < 16 || a->fec_stride > LC3FEC_MAX_PKT || (a->fec_stride & 15)) return LC3_ERROR;
    if (a->passes < 1 || a->passes > LC3REP_MAX_PASSES) return LC3_ERROR;
    const long long nh = (long long)n_streams * a->med_slots, np = (long long)n_streams * a->fec_slots;
    if (nh >= LC3FEC_MAX_PACKETS || np >= LC3FEC_MAX_PACKETS) return LC3_ERROR;
    if (a->med_offset > a->ring_capacity - nh * a->med_stride) return LC3_ERROR;                  /* the history ends behind the ring */
    /* fec_store, the history's range of the ring and the metadata arrays lie apart */
    const uintptr_t at[8] = {(uintptr_t)a->ring + (uintptr_t)a->med_offset, (uintptr_t)a->fec_store, (uintptr_t)a->med_seq, (uintptr_t)a->med_size, (uintptr_t)a->cell_seq,
                             (uintptr_t)a->cell_size, (uintptr_t)a->cell_status, (uintptr_t)a->state};
    const uintptr_t len[8] = {(uintptr_t)(nh * a->med_stride), (uintptr_t)(np * a->fec_stride), 4 * (uintptr_t)nh, 4 * (uintptr_t)nh, 4 * (uintptr_t)np, 4 * (uintptr_t)np,
                              (uintptr_t)np, sizeof(int32_t) * LC3REP_STATE_WORDS * (uintptr_t)n_streams};
    for (int i = 0; i < 8; i++)
        for (int j = i + 1; j < 8; j++)
            if (at[i] < at[j] + len[j] && at[j] < at[i] + len[i]) return LC3_ERROR;
    if ((uintptr_t)a->work & 7) return LC3_ERROR;
    return LC3_OK;
}
static lc3rep_io fec_repair_io(const fec_repair_args* a, int n_streams)
{
    const lc3rep_io q = {(uint8_t*)a->ring, (const long long*)a->dg_offsets, a->dg_sizes, a->stream, a->seq, a->fec_stream, (const long long*)a->fec_offsets,
                         a->fec_num_bytes, a->fec_seq, a->ssrc, a->med_seq, a->med_size, (uint8_t*)a->fec_store, a->cell_seq, a->cell_size, a->cell_status, a->state,
                         (long long*)a->rec_dg_offsets, a->rec_dg_sizes, a->rec_seq, a->item_status, a->fec_status, a->stats, (long long)a->ring_capacity,
                         a->n_items > 0 ? (long long)a->n_items : 0, a->n_fec > 0 ? (long long)a->n_fec : 0, (long long)a->med_offset, n_streams, a->med_slots,
                         a->med_stride, a->fec_slots, a->fec_stride, a->passes};
    return q;
}
#define FEC_REPAIR_PARAMS \
    int64_t n_items, void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes, const int32_t* stream, const int32_t* seq, \
    int64_t n_fec, const int32_t* fec_stream, const int64_t* fec_offsets, const int32_t* fec_num_bytes, const int32_t* fec_seq, const int32_t* ssrc, \
    int64_t med_offset, int med_slots, int med_stride, int32_t* med_seq, int32_t* med_size, \
    void* fec_store, int fec_slots, int fec_stride, int32_t* cell_seq, int32_t* cell_size, uint8_t* cell_status, int32_t* state, int passes, \
    int64_t* rec_dg_offsets, int32_t* rec_dg_sizes, int32_t* rec_seq, uint8_t* item_status, uint8_t* fec_status, int32_t* stats, void* work
#define FEC_REPAIR_ARGS \
    {n_items, ring, ring_capacity, dg_offsets, dg_sizes, stream, seq, n_fec, fec_stream, fec_offsets, fec_num_bytes, fec_seq, ssrc, med_offset, med_slots, med_stride, \
     med_seq, med_size, fec_store, fec_slots, fec_stride, cell_seq, cell_size, cell_status, state, passes, rec_dg_offsets, rec_dg_sizes, rec_seq, item_status, fec_status, \
     stats, work}
int64_t lc3plus_fec_repair_work_bytes(int n_streams, int med_slots, int fec_slots)
{
    if (n_streams <= 0 || !pow2_in(med_slots, LC3REP_MIN_MED, LC3REP_MAX_MED) || !pow2_in(fec_slots, LC3REP_MIN_CELLS, LC3REP_MAX_CELLS)) return 0;
    if ((long long)n_streams * med_slots >= LC3FEC_MAX_PACKETS || (long long)n_streams * fec_slots >= LC3FEC_MAX_PACKETS) return 0;
    return lc3rep_work_bytes(n_streams, med_slots, fec_slots);
}
/* the rule on the host: the kernels' steps (lc3_repair.inc) one after the other, on the text they run and over the same workspace */
LC3_Error lc3plus_plan_fec_repair(int n_streams, FEC_REPAIR_PARAMS, void* hip_stream, int sync)
{
    (void)hip_stream; (void)sync;
    const fec_repair_args a = FEC_REPAIR_ARGS;
    const LC3_Error e = fec_repair_check(&a, n_streams > 0 ? n_streams : 0);
    if (e) return e;
    const lc3rep_io q = fec_repair_io(&a, n_streams);
    const lc3rep_work w = lc3rep_work_of(work, n_streams, med_slots, fec_slots);
    const long long nh = (long long)n_streams * med_slots, np = (long long)n_streams * fec_slots, items = q.n_items + q.n_fec;
    /* fill */
    for (long long i = 0; i < 2LL * n_streams; i++) { w.first[i] = LC3FEC_NO_ENTRY; w.dist[i] = 0; }
    for (long long i = 0; i < nh; i++) w.mclaim[i] = w.tclaim[i] = LC3FEC_NO_ENTRY;
    for (long long i = 0; i < np; i++) { w.fclaim[i] = LC3FEC_NO_ENTRY; rec_dg_offsets[i] = 0; rec_dg_sizes[i] = 0; rec_seq[i] = 0; }
    for (int i = 0; i < LC3REP_PROG_WORDS; i++) w.prog[i] = i == 0;
    if (stats) memset(stats, 0, sizeof(int32_t) * LC3FEC_STATS_WORDS);
    for (long long i = 0; i < items; i++) lc3rep_first_step(&q, &w, i);
    for (long long i = 0; i < items; i++) lc3rep_dist_step(&q, &w, i);
    for (long long i = 0; i < items; i++) lc3rep_claim_step(&q, &w, i);
    for (long long i = 0; i < nh; i++) lc3rep_settle_step(&q, &w, LC3REP_MED, i);
    for (long long i = 0; i < np; i++) lc3rep_settle_step(&q, &w, LC3REP_FEC, i);
    /* copy */
    for (long long i = 0; i < items; i++) {
        const lc3rep_item it = lc3rep_item_of(&q, i);
        long long slot = 0;
        const int st = lc3rep_place_step(&q, &w, &it, &slot);
        if (it.kind == LC3REP_MED && item_status) item_status[i] = (uint8_t)st;
        if (st != LC3REP_STORED) continue;
        memcpy(it.kind == LC3REP_FEC ? q.fec_store + lc3rep_cell_at(&q, slot) : q.ring + lc3rep_slot_at(&q, slot), q.ring + it.off, (size_t)it.size);
    }
    for (int p = 1; p <= passes; p++) {
        if (!w.prog[p - 1]) break;                                    /* a pass behind one that rebuilt nothing changes nothing */
        for (long long c = 0; c < np; c++) {
            const int st = lc3rep_verdict_step(&q, &w, p, c);
            if (stats && st > 0 && st != LC3FEC_MISSING && lc3rep_carried(&w, c)) stats[st]++;
        }
        if (!w.prog[p]) continue;
        for (long long c = 0; c < np; c++) {
            lc3fec_item h;
            long long k = 0;
            uint32_t sn = 0;
            const int st = lc3rep_rebuild_claim(&q, &w, c, &h, &k, &sn);
            if (st >= 0 && stats && lc3rep_carried(&w, c)) stats[st]++;
            if (st != LC3FEC_RECOVERED) continue;
            const int s = (int)(c / fec_slots);
            uint32_t hdr = 0, ts = 0, len = 0;
            for (int i = 0; i < LC3FEC_MAX_BITS; i++) {
                const uint32_t mine = (h.sn + (uint32_t)i) & 0xFFFFu;
                uint32_t mh, mt, ml;
                if (!(h.mask >> (LC3FEC_MAX_BITS - 1 - i) & 1) || mine == sn) continue;
                lc3rep_member_fields(&q, (long long)s * med_slots + (mine & (uint32_t)(med_slots - 1)), &mh, &mt, &ml);
                hdr ^= mh; ts ^= mt; len ^= ml;
            }
            const int rl = lc3rep_rebuild_header(&q, c, &h, k, sn, hdr, ts, len);
            uint8_t* dst = q.ring + lc3rep_slot_at(&q, k) + LC3R_FIXED;
            memcpy(dst, q.fec_store + lc3rep_cell_at(&q, c) + h.hl, (size_t)rl);
            for (int i = 0; i < LC3FEC_MAX_BITS; i++) {
                const uint32_t mine = (h.sn + (uint32_t)i) & 0xFFFFu;
                if (!(h.mask >> (LC3FEC_MAX_BITS - 1 - i) & 1) || mine == sn) continue;
                const long long m = (long long)s * med_slots + (mine & (uint32_t)(med_slots - 1));
                fec_xor(dst, q.ring + lc3rep_slot_at(&q, m) + LC3R_FIXED, IMIN(med_size[m] - LC3R_FIXED, rl));
            }
        }
    }
    /* report */
    for (long long f = 0; f < q.n_fec; f++) {
        const int st = lc3rep_report_step(&q, &w, f);
        if (stats) stats[st]++;
    }
    for (int s = 0; s < n_streams; s++) lc3rep_state_step(&q, &w, s);
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_fec_repair(lc3plus_dec_batch* b, FEC_REPAIR_PARAMS, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    const fec_repair_args a = FEC_REPAIR_ARGS;
    const lc3host_view v = lc3host_dec_view(b);
    const LC3_Error e = fec_repair_check(&a, v.n_streams);
    if (e) return e;
    lc3rep_call q;
    memset(&q, 0, sizeof q);
    q.sync = sync; q.io = fec_repair_io(&a, v.n_streams); q.work = work;
    return SIBLING_RUN(lc3rep_call, SIB_REPAIR, 0, v, hip_stream, &q);
}
/* ---- reception reports (include/lc3plus_batch.h "Reception reports"; lc3_rtcp_shim.h) ---- */
/* what a stats call takes behind its batch, in the header's order */
typedef struct {
    int64_t n_items; const int32_t* stream; const int32_t* seq; const int32_t* timestamp; const int32_t* arrival;
    int n_streams; const int32_t* state_in; int32_t* state_out;
    int make_report; const int32_t* ssrc; const int32_t* lsr; const int32_t* dlsr; uint8_t* blocks;
    int32_t* ext_seq; uint8_t* item_status; int32_t* stream_stats;
} rtcp_stats_args;
#define RTCP_STATS_PARAMS \
    int64_t n_items, const int32_t* stream, const int32_t* seq, const int32_t* timestamp, const int32_t* arrival, \
    int n_streams, const int32_t* state_in, int32_t* state_out, \
    int make_report, const int32_t* ssrc, const int32_t* lsr, const int32_t* dlsr, uint8_t* blocks, \
    int32_t* ext_seq, uint8_t* item_status, int32_t* stream_stats
#define RTCP_STATS_ARGS \
    {n_items, stream, seq, timestamp, arrival, n_streams, state_in, state_out, make_report, ssrc, lsr, dlsr, blocks, ext_seq, item_status, stream_stats}
/* the checks every stats call makes first, in the header's order */
static LC3_Error rtcp_stats_check(const rtcp_stats_args* a)
{
    if (!a->stream || !a->seq || !a->timestamp || !a->arrival || !a->state_in || !a->state_out) return LC3_NULL_ERROR;
    if (a->make_report && (!a->ssrc || !a->blocks)) return LC3_NULL_ERROR;
    if (a->n_items <= 0 || a->n_items >= LC3Q_MAX_ITEMS || a->n_streams <= 0 || (a->make_report != 0 && a->make_report != 1)) return LC3_ERROR;
    return LC3_OK;
}
int64_t lc3plus_rtcp_workspace_bytes(int64_t n_items, int n_streams)
{
    return (int64_t)lc3q_workspace_bytes((long long)n_items, n_streams);
}
/* the rule on the host: the list once in its order, every item on its stream's state, then the reports */
LC3_Error lc3plus_plan_rtcp_stats(RTCP_STATS_PARAMS)
{
    const rtcp_stats_args a = RTCP_STATS_ARGS;
    const LC3_Error e = rtcp_stats_check(&a);
    if (e) return e;
    if (state_out != state_in) memmove(state_out, state_in, sizeof(int32_t) * LC3Q_STATE_WORDS * (size_t)n_streams);
    if (stream_stats) memset(stream_stats, 0, sizeof(int32_t) * LC3Q_STATS_WORDS * (size_t)n_streams);
    for (int64_t i = 0; i < n_items; i++) {
        const int s = stream[i];
        uint32_t ext = 0;
        int st = LC3Q_DROPPED;
        if (s >= 0 && s < n_streams) {
            lc3q_state v;
            memcpy(v.w, state_out + (size_t)s * LC3Q_STATE_WORDS, sizeof v.w);
            st = lc3q_step(&v, (uint32_t)seq[i], (uint32_t)arrival[i] - (uint32_t)timestamp[i], &ext);
            memcpy(state_out + (size_t)s * LC3Q_STATE_WORDS, v.w, sizeof v.w);
            if (stream_stats) {
                int32_t* t = stream_stats + (size_t)s * LC3Q_STATS_WORDS;
                t[LC3Q_ST_COUNTED] += st != LC3Q_JUMP; t[LC3Q_ST_JUMP] += st == LC3Q_JUMP; t[LC3Q_ST_RESTART] += st == LC3Q_RESTART;
                t[LC3Q_ST_REORDERED] += st == LC3Q_REORDERED;
            }
        }
        if (item_status) item_status[i] = (uint8_t)st;
        if (ext_seq) ext_seq[i] = (int32_t)ext;
    }
    if (make_report)
        for (int s = 0; s < n_streams; s++) {
            lc3q_state v;
            uint32_t blk[LC3Q_BLOCK_WORDS];
            memcpy(v.w, state_out + (size_t)s * LC3Q_STATE_WORDS, sizeof v.w);
            lc3q_report(&v, (uint32_t)ssrc[s], lsr ? (uint32_t)lsr[s] : 0u, dlsr ? (uint32_t)dlsr[s] : 0u, blk);
            memcpy(state_out + (size_t)s * LC3Q_STATE_WORDS, v.w, sizeof v.w);
            lc3q_block_out(blocks + (size_t)s * LC3Q_BLOCK_BYTES, blk);
        }
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_rtcp_stats(lc3plus_dec_batch* b, RTCP_STATS_PARAMS, void* workspace, int64_t workspace_bytes, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    const rtcp_stats_args a = RTCP_STATS_ARGS;
    if (!workspace) return LC3_NULL_ERROR;
    const LC3_Error e = rtcp_stats_check(&a);
    if (e) return e;
    if (workspace_bytes < lc3plus_rtcp_workspace_bytes(n_items, n_streams)) return LC3_ERROR;
    lc3rtcp_stats_call q;
    memset(&q, 0, sizeof q);
    q.n_streams = n_streams; q.make_report = make_report; q.sync = sync; q.n_items = (long long)n_items;
    q.stream = stream; q.seq = seq; q.timestamp = timestamp; q.arrival = arrival; q.state_in = state_in; q.state_out = state_out;
    q.ssrc = ssrc; q.lsr = lsr; q.dlsr = dlsr; q.blocks = blocks; q.ext_seq = ext_seq; q.item_status = item_status; q.stream_stats = stream_stats;
    q.workspace = workspace; q.workspace_bytes = (long long)workspace_bytes;
    return SIBLING_RUN(lc3rtcp_stats_call, SIB_RTCP, 0, lc3host_dec_view(b), hip_stream, &q);
}
/* ---- Secure RTP (include/lc3plus_batch.h "Secure RTP"; lc3_srtp_shim.h) ---- */
LC3_Error lc3plus_srtp_make_context(const uint8_t* master_key, const uint8_t* master_salt, int32_t* ctx)
{
    if (!master_key || !master_salt || !ctx) return LC3_NULL_ERROR;
    lc3s_make_context(master_key, master_salt, ctx);
    return LC3_OK;
}
/* A suite of Secure RTP as the calls below take it: its sibling, the two tag lengths it accepts, the words of a context, and its two rules under one
 * signature for the host plans (te: Te0; a rule that knows its tag length does not read the argument) */
typedef struct {
    int sibling, tag_len[2], ctx_words;
    int (*protect)(const lc3s_protect_in* q, long long p, const uint32_t* te, int32_t* out_size);
    int (*unprotect)(uint8_t* ring, long long off, int32_t size, int tag_len, const lc3s_item* it, const int32_t* state, uint32_t s_l_first, const uint32_t* ctx,
                     const uint32_t* te, long long* index);
} srtp_suite;
static int hmac_protect(const lc3s_protect_in* q, long long p, const uint32_t* te, int32_t* out_size) { return lc3s_protect(q, p, te, 1, out_size); }
static int hmac_unprotect(uint8_t* ring, long long off, int32_t size, int tag_len, const lc3s_item* it, const int32_t* state, uint32_t s_l_first, const uint32_t* ctx,
                          const uint32_t* te, long long* index)
{
    return lc3s_unprotect(ring, off, size, tag_len, it, state, s_l_first, ctx, te, 1, index);
}
static int gcm_protect(const lc3s_protect_in* q, long long p, const uint32_t* te, int32_t* out_size) { return lc3g_protect(q, p, te, 1, NULL, 1, out_size); }
static int gcm_unprotect(uint8_t* ring, long long off, int32_t size, int tag_len, const lc3s_item* it, const int32_t* state, uint32_t s_l_first, const uint32_t* ctx,
                         const uint32_t* te, long long* index)
{
    return lc3g_unprotect(ring, off, size, it, state, s_l_first, ctx, te, 1, NULL, 1, index);
}
static const srtp_suite SUITE_HMAC = {SIB_SRTP, {4, 10}, LC3S_CTX_WORDS, hmac_protect, hmac_unprotect};
static const srtp_suite SUITE_GCM = {SIB_GCM, {LC3G_TAG_BYTES, LC3G_TAG_BYTES}, LC3G_CTX_WORDS, gcm_protect, gcm_unprotect};      /* the GCM calls pass LC3G_TAG_BYTES */
static int srtp_tag_ok(const srtp_suite* u, int tag_len) { return tag_len == u->tag_len[0] || tag_len == u->tag_len[1]; }

/* what a protect call takes behind its batch, in the header's order */
typedef struct {
    int64_t max_packets; const int64_t* n_packets;
    const int32_t* pkt_route; const int64_t* pkt_offset; const int32_t* pkt_size; const uint8_t* pkt_status;
    const void* wire; int64_t wire_capacity; int header_room; int payload_room;
    int n_routes; const int32_t* ctx; const int32_t* roc; const int32_t* seq_base; const int32_t* next_seq;
    void* dst; int64_t dst_capacity; int64_t dst_stride; int tag_len;
    int64_t* out_offset; int32_t* out_size; uint8_t* out_status; int32_t* next_roc;
} srtp_protect_args;
/* the checks every protect call makes first, in the header's order */
static LC3_Error srtp_protect_check(const srtp_suite* u, const srtp_protect_args* a)
{
    if (!a->n_packets || !a->pkt_route || !a->pkt_offset || !a->pkt_size || !a->pkt_status || !a->wire || !a->ctx || !a->roc || !a->seq_base || !a->dst ||
        !a->out_offset || !a->out_size || !a->out_status)
        return LC3_NULL_ERROR;
    if (a->next_roc && !a->next_seq) return LC3_NULL_ERROR;
    if (a->max_packets <= 0 || a->max_packets >= LC3S_MAX_ITEMS || a->wire_capacity < 0 || a->payload_room < 0 || a->header_room < LC3R_FIXED ||
        a->header_room - LC3R_FIXED < a->payload_room || a->n_routes <= 0)
        return LC3_ERROR;
    if (a->dst_capacity < 0 || a->dst_stride <= 0 || a->dst_stride > LC3S_MAX_STRIDE || !srtp_tag_ok(u, a->tag_len)) return LC3_ERROR;
    const uintptr_t w0 = (uintptr_t)a->wire, d0 = (uintptr_t)a->dst;
    if (d0 < w0 + (uintptr_t)a->wire_capacity && w0 < d0 + (uintptr_t)a->dst_capacity) return LC3_ERROR;          /* out of place only */
    return LC3_OK;
}
static lc3s_protect_in srtp_protect_in(const srtp_protect_args* a)
{
    const lc3s_protect_in q = {a->pkt_route, (const long long*)a->pkt_offset, a->pkt_size, a->pkt_status, (const uint8_t*)a->wire, a->ctx, a->roc, a->seq_base,
                               a->next_seq, (uint8_t*)a->dst, (long long)a->wire_capacity, (long long)a->dst_capacity, (long long)a->dst_stride, a->header_room,
                               a->payload_room, a->n_routes, a->tag_len};
    return q;
}
/* the checks, then the rule on the host: the kernels' steps (lc3_srtp_suite.inc) on the text they run */
static LC3_Error srtp_protect_plan(const srtp_suite* u, const srtp_protect_args* a)
{
    const LC3_Error e = srtp_protect_check(u, a);
    if (e) return e;
    const lc3s_protect_in q = srtp_protect_in(a);
    uint32_t te[LC3S_TE_WORDS];
    for (uint32_t x = 0; x < LC3S_TE_WORDS; x++) te[x] = lc3s_te0(x);
    const int64_t n = *a->n_packets < a->max_packets ? *a->n_packets : a->max_packets;
    for (int64_t p = 0; p < n; p++) {
        int32_t size = 0;
        const int st = u->protect(&q, p, te, &size);
        a->out_offset[p] = p * a->dst_stride; a->out_size[p] = size; a->out_status[p] = (uint8_t)st;
    }
    if (a->next_roc)
        for (int r = 0; r < a->n_routes; r++) lc3s_route_out(&q, r, a->next_roc);
    return LC3_OK;
}
/* what an unprotect call takes behind its batch, in the header's order */
typedef struct {
    int64_t n_items; void* ring; int64_t ring_capacity; const int64_t* dg_offsets; const int32_t* dg_sizes;
    int n_ssrc; const int32_t* ssrc_key; const int32_t* ctx; const int32_t* state_in; int32_t* state_out; int tag_len;
    int32_t* sizes_out; uint8_t* status; int64_t* index; int32_t* stats;
} srtp_unprotect_args;
static LC3_Error srtp_unprotect_check(const srtp_suite* u, const srtp_unprotect_args* a)
{
    if (!a->ring || !a->dg_offsets || !a->dg_sizes || !a->ssrc_key || !a->ctx || !a->state_in || !a->state_out || !a->sizes_out) return LC3_NULL_ERROR;
    if (a->n_items <= 0 || a->n_items >= LC3S_MAX_ITEMS || a->ring_capacity < 0 || a->n_ssrc <= 0 || !srtp_tag_ok(u, a->tag_len)) return LC3_ERROR;
    return LC3_OK;
}
int64_t lc3plus_srtp_workspace_bytes(int64_t n_items, int n_ssrc)
{
    return (int64_t)lc3s_workspace_bytes((long long)n_items, n_ssrc);
}
/* the checks, then the rule on the host: the kernels' passes one after the other - the first items, the items against state_in, the window bits against the
 * new tops, the state */
static LC3_Error srtp_unprotect_plan(const srtp_suite* u, const srtp_unprotect_args* a)
{
    const LC3_Error e = srtp_unprotect_check(u, a);
    if (e) return e;
    const int64_t n_items = a->n_items;
    const int n_ssrc = a->n_ssrc, tag_len = a->tag_len;
    uint32_t te[LC3S_TE_WORDS];
    for (uint32_t x = 0; x < LC3S_TE_WORDS; x++) te[x] = lc3s_te0(x);
    unsigned long long* top1 = calloc((size_t)n_ssrc, sizeof *top1);
    unsigned long long* bits = calloc((size_t)n_ssrc, sizeof *bits);
    int64_t* first = malloc(sizeof *first * (size_t)n_ssrc);
    int64_t* accepted = malloc(sizeof *accepted * (size_t)n_items);
    lc3s_item* items = malloc(sizeof *items * (size_t)n_items);
    if (!top1 || !bits || !first || !accepted || !items) { free(top1); free(bits); free(first); free(accepted); free(items); return LC3_ERROR; }
    uint8_t* r8 = (uint8_t*)a->ring;
    for (int s = 0; s < n_ssrc; s++) first[s] = -1;
    if (a->stats) memset(a->stats, 0, sizeof(int32_t) * LC3S_STATS_WORDS);
    for (int64_t i = 0; i < n_items; i++) {
        items[i] = lc3s_check(r8, a->ring_capacity, a->dg_offsets[i], a->dg_sizes[i], tag_len, a->ssrc_key, n_ssrc);
        if (items[i].status == LC3S_OK && first[items[i].src] < 0) first[items[i].src] = i;
    }
    for (int64_t i = 0; i < n_items; i++) {
        int st = items[i].status;
        long long idx = 0;
        accepted[i] = -1;
        a->sizes_out[i] = 0;
        if (st == LC3S_OK) {
            const int s = items[i].src;
            const int32_t* state = a->state_in + (size_t)s * LC3S_STATE_WORDS;
            const uint32_t s_l_first = lc3s_seq_at(r8, a->dg_offsets[first[s]]);
            st = u->unprotect(r8, a->dg_offsets[i], a->dg_sizes[i], tag_len, &items[i], state, s_l_first, (const uint32_t*)a->ctx + (size_t)s * (size_t)u->ctx_words, te, &idx);
            if (st == LC3S_OK) {
                accepted[i] = idx; a->sizes_out[i] = a->dg_sizes[i] - tag_len;
                if ((unsigned long long)idx + 1 > top1[s]) top1[s] = (unsigned long long)idx + 1;
            }
        }
        if (a->status) a->status[i] = (uint8_t)st;
        if (a->index) a->index[i] = idx;
        if (a->stats) a->stats[st]++;
    }
    for (int64_t i = 0; i < n_items; i++)
        if (accepted[i] >= 0) {
            const int s = items[i].src;
            bits[s] |= lc3s_window_bit(a->state_in + (size_t)s * LC3S_STATE_WORDS, top1[s], accepted[i]);
        }
    for (int s = 0; s < n_ssrc; s++) lc3s_state_out(a->state_in + (size_t)s * LC3S_STATE_WORDS, a->state_out + (size_t)s * LC3S_STATE_WORDS, top1[s], bits[s]);
    free(top1); free(bits); free(first); free(accepted); free(items);
    return LC3_OK;
}
/* every protect entry point of a batch ends here: the checks, then the suite's sibling */
static LC3_Error srtp_protect_queue(const srtp_suite* u, lc3host_view v, const srtp_protect_args* a, void* hip_stream, int sync)
{
    const LC3_Error e = srtp_protect_check(u, a);
    if (e) return e;
    lc3srtp_protect_call q;
    memset(&q, 0, sizeof q);
    q.sync = sync; q.max_packets = (long long)a->max_packets; q.n_packets = (const long long*)a->n_packets; q.in = srtp_protect_in(a);
    q.out_offset = (long long*)a->out_offset; q.out_size = a->out_size; q.out_status = a->out_status; q.next_roc = a->next_roc;
    return SIBLING_RUN(lc3srtp_protect_call, u->sibling, 0, v, hip_stream, &q);
}
/* both unprotect entry points end here, behind the check of the batch: the workspace's pointer, the checks, the workspace's size, then the suite's sibling */
static LC3_Error srtp_unprotect_queue(const srtp_suite* u, lc3host_view v, const srtp_unprotect_args* a, void* workspace, int64_t workspace_bytes, void* hip_stream,
                                      int sync)
{
    if (!workspace) return LC3_NULL_ERROR;
    const LC3_Error e = srtp_unprotect_check(u, a);
    if (e) return e;
    if (workspace_bytes < lc3plus_srtp_workspace_bytes(a->n_items, a->n_ssrc)) return LC3_ERROR;
    lc3srtp_unprotect_call q;
    memset(&q, 0, sizeof q);
    q.sync = sync; q.n_ssrc = a->n_ssrc; q.tag_len = a->tag_len; q.n_items = (long long)a->n_items; q.ring_capacity = (long long)a->ring_capacity;
    q.ring = a->ring; q.dg_offsets = (const long long*)a->dg_offsets; q.dg_sizes = a->dg_sizes; q.ssrc_key = a->ssrc_key; q.ctx = a->ctx; q.state_in = a->state_in;
    q.state_out = a->state_out; q.sizes_out = a->sizes_out; q.status = a->status; q.index = (long long*)a->index; q.stats = a->stats;
    q.workspace = workspace; q.workspace_bytes = (long long)workspace_bytes;
    return SIBLING_RUN(lc3srtp_unprotect_call, u->sibling, 1, v, hip_stream, &q);
}
/* the ten entry points: the arguments in the header's order into the struct, then the suite.  The GCM calls take the HMAC calls' lists without tag_len, which
 * stands between HEAD and TAIL, and put LC3G_TAG_BYTES in its place */
#define SRTP_PROTECT_HEAD \
    int64_t max_packets, const int64_t* n_packets, \
    const int32_t* pkt_route, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_status, \
    const void* wire, int64_t wire_capacity, int header_room, int payload_room, \
    int n_routes, const int32_t* ctx, const int32_t* roc, const int32_t* seq_base, const int32_t* next_seq, \
    void* dst, int64_t dst_capacity, int64_t dst_stride
#define SRTP_PROTECT_TAIL int64_t* out_offset, int32_t* out_size, uint8_t* out_status, int32_t* next_roc
#define SRTP_PROTECT_PARAMS SRTP_PROTECT_HEAD, int tag_len, SRTP_PROTECT_TAIL
#define GCM_PROTECT_PARAMS SRTP_PROTECT_HEAD, SRTP_PROTECT_TAIL
#define SRTP_PROTECT_ARGS(tag) {max_packets, n_packets, pkt_route, pkt_offset, pkt_size, pkt_status, wire, wire_capacity, header_room, payload_room, n_routes, ctx, \
                                roc, seq_base, next_seq, dst, dst_capacity, dst_stride, tag, out_offset, out_size, out_status, next_roc}
#define SRTP_UNPROTECT_HEAD \
    int64_t n_items, void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes, \
    int n_ssrc, const int32_t* ssrc_key, const int32_t* ctx, const int32_t* state_in, int32_t* state_out
#define SRTP_UNPROTECT_TAIL int32_t* sizes_out, uint8_t* status, int64_t* index, int32_t* stats
#define SRTP_UNPROTECT_PARAMS SRTP_UNPROTECT_HEAD, int tag_len, SRTP_UNPROTECT_TAIL
#define GCM_UNPROTECT_PARAMS SRTP_UNPROTECT_HEAD, SRTP_UNPROTECT_TAIL
#define SRTP_UNPROTECT_ARGS(tag) {n_items, ring, ring_capacity, dg_offsets, dg_sizes, n_ssrc, ssrc_key, ctx, state_in, state_out, tag, sizes_out, status, index, stats}
LC3_Error lc3plus_plan_srtp_protect(SRTP_PROTECT_PARAMS)
{
    const srtp_protect_args a = SRTP_PROTECT_ARGS(tag_len);
    return srtp_protect_plan(&SUITE_HMAC, &a);
}
LC3_Error lc3plus_plan_srtp_unprotect(SRTP_UNPROTECT_PARAMS)
{
    const srtp_unprotect_args a = SRTP_UNPROTECT_ARGS(tag_len);
    return srtp_unprotect_plan(&SUITE_HMAC, &a);
}
BATCH_TWINS(srtp_protect, SRTP_PROTECT_PARAMS, srtp_protect_args, SRTP_PROTECT_ARGS(tag_len), srtp_protect_queue(&SUITE_HMAC, v, &a, hip_stream, sync))
LC3_Error lc3plus_dec_batch_srtp_unprotect(lc3plus_dec_batch* b, SRTP_UNPROTECT_PARAMS, void* workspace, int64_t workspace_bytes, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    const srtp_unprotect_args a = SRTP_UNPROTECT_ARGS(tag_len);
    return srtp_unprotect_queue(&SUITE_HMAC, lc3host_dec_view(b), &a, workspace, workspace_bytes, hip_stream, sync);
}
/* ---- Secure RTP, AEAD (include/lc3plus_batch.h "Secure RTP, AEAD"; lc3_gcm_shim.h): the calls above with SUITE_GCM ---- */
LC3_Error lc3plus_srtp_gcm_make_context(const uint8_t* master_key, int key_bytes, const uint8_t* master_salt, int32_t* ctx)
{
    if (!master_key || !master_salt || !ctx) return LC3_NULL_ERROR;
    if (key_bytes != 16 && key_bytes != 32) return LC3_ERROR;
    lc3g_make_context(master_key, key_bytes, master_salt, ctx);
    return LC3_OK;
}
LC3_Error lc3plus_plan_srtp_gcm_protect(GCM_PROTECT_PARAMS)
{
    const srtp_protect_args a = SRTP_PROTECT_ARGS(LC3G_TAG_BYTES);
    return srtp_protect_plan(&SUITE_GCM, &a);
}
BATCH_TWINS(srtp_gcm_protect, GCM_PROTECT_PARAMS, srtp_protect_args, SRTP_PROTECT_ARGS(LC3G_TAG_BYTES), srtp_protect_queue(&SUITE_GCM, v, &a, hip_stream, sync))
LC3_Error lc3plus_plan_srtp_gcm_unprotect(GCM_UNPROTECT_PARAMS)
{
    const srtp_unprotect_args a = SRTP_UNPROTECT_ARGS(LC3G_TAG_BYTES);
    return srtp_unprotect_plan(&SUITE_GCM, &a);
}
LC3_Error lc3plus_dec_batch_srtp_gcm_unprotect(lc3plus_dec_batch* b, GCM_UNPROTECT_PARAMS, void* workspace, int64_t workspace_bytes, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    const srtp_unprotect_args a = SRTP_UNPROTECT_ARGS(LC3G_TAG_BYTES);
    return srtp_unprotect_queue(&SUITE_GCM, lc3host_dec_view(b), &a, workspace, workspace_bytes, hip_stream, sync);
}
