/* stub_shim.c -- every lc3hip_* symbol of audio_codec_amd/csrc/lc3_shim.h as a function that touches no GPU.
 *
 * Linked with lc3_host.c and lc3_packet.c in place of lc3_runtime.hip and the kernels (csrc/Makefile, target stub), it lets the host logic - which pointer, which slice of
 * which array, which result, which thread - be tested on a machine without a device: every create succeeds, every call returns success and appends one
 * record to a log that lc3stub_log() returns; lc3stub_fail_ctx() makes the encode / decode / state calls of one context fail.  Contexts are numbered in
 * the order they are created, from 0 after lc3stub_reset().  Never part of the product library.
 *
 * Configuration traffic - the uploads and downloads of the per-stream configuration, the stream-lifecycle calls and the calls whose rates or sizes are in device
 * memory - goes into a second log, off until lc3stub_cfg_enable(1): lines of text, one JSON object per stub call in the order the calls were made, with named
 * fields and of every uploaded entry the words the host sets.  A call that also appends to the first log leaves a line {"ctx", "call", "rec": its index there}, so
 * that the two logs can be read as one sequence (tests/test_host_calls_cpu.py).  lc3stub_rec and the first log are as they were. */
#include <pthread.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../audio_codec_amd/csrc/lc3_shim.h"

enum { STUB_ENCODE = 1, STUB_DECODE = 2, STUB_GET_STATE = 3, STUB_SET_STATE = 4, STUB_WAIT = 5, STUB_PLACEMENT = 6, STUB_COUNTS = 7 };
#define STUB_STATE_BYTES 32          /* per channel-stream */

/* p: encode pcm, out; decode frames, pcm, status, bfi; state: the host pointer.  a / b: the first two words and the last one of the two per-frame arrays
 * the call was given (encode: frame sizes, bandwidths in force; decode: sizes, loss flags), -1 where there is none.  sync / on_device as passed.
 * STUB_PLACEMENT (lc3hip_set_pcm_placement, lc3hip_dec_set_pcm_placement): p[0] the offsets pointer, a[0] the capacity.
 * STUB_COUNTS (lc3hip_set_frame_counts, lc3hip_dec_set_frame_counts): p[0] the counts pointer. */
typedef struct {
    int32_t ctx, kind, dec, n_frames, stride, fmt, on_device, sync;
    uint64_t p[4];
    int64_t a[3], b[3];
    uint64_t bytes, hip_stream;
} lc3stub_rec;

typedef struct { int id, dec, n_streams, channels; } stub_ctx;

static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;
static lc3stub_rec* g_log; static int g_n, g_cap, g_next_ctx, g_fail = -1, g_device_args;

/* the second log: text, grown as needed; a line that does not fit the memory there is is dropped */
static char* g_cfg; static size_t g_cfg_n, g_cfg_cap; static int g_cfg_on;
static const char* const stub_kind_names[] = {"?", "encode", "decode", "get_state", "set_state", "wait", "placement", "counts"};
static void cfg_put_locked(const char* fmt, va_list ap)
{
    char line[512];
    const int n = vsnprintf(line, sizeof line, fmt, ap);
    if (n <= 0 || (size_t)n >= sizeof line) return;
    if (g_cfg_n + (size_t)n + 1 > g_cfg_cap) {
        const size_t cap = 2 * g_cfg_cap + 4096;
        char* q = (char*)realloc(g_cfg, cap);
        if (!q) return;
        g_cfg = q; g_cfg_cap = cap;
    }
    memcpy(g_cfg + g_cfg_n, line, (size_t)n + 1);
    g_cfg_n += (size_t)n;
}
/* (g_mu held) */
static void cfg_put(const char* fmt, ...) { va_list ap; va_start(ap, fmt); cfg_put_locked(fmt, ap); va_end(ap); }
void lc3stub_cfg_enable(int on) { pthread_mutex_lock(&g_mu); g_cfg_on = on; pthread_mutex_unlock(&g_mu); }
/* copies up to max bytes of the text, oldest first, no terminator; returns how many the log holds */
size_t lc3stub_cfg_log(char* out, size_t max)
{
    pthread_mutex_lock(&g_mu);
    const size_t n = g_cfg_n;
    if (out && n) memcpy(out, g_cfg, n < max ? n : max);
    pthread_mutex_unlock(&g_mu);
    return n;
}

void lc3stub_reset(void)
{
    pthread_mutex_lock(&g_mu);
    g_n = 0; g_next_ctx = 0; g_fail = -1; g_device_args = 0; g_cfg_n = 0;
    pthread_mutex_unlock(&g_mu);
}
void lc3stub_fail_ctx(int ctx) { pthread_mutex_lock(&g_mu); g_fail = ctx; pthread_mutex_unlock(&g_mu); }
void lc3stub_device_args(int on) { pthread_mutex_lock(&g_mu); g_device_args = on; pthread_mutex_unlock(&g_mu); }
int lc3stub_rec_sizeof(void) { return (int)sizeof(lc3stub_rec); }
/* copies up to max records, oldest first; returns how many the log holds */
int lc3stub_log(lc3stub_rec* out, int max)
{
    pthread_mutex_lock(&g_mu);
    const int n = g_n;
    if (out) memcpy(out, g_log, sizeof(lc3stub_rec) * (size_t)(n < max ? n : max));
    pthread_mutex_unlock(&g_mu);
    return n;
}
/* appends the record; returns 1 where the context is the one chosen to fail */
static int stub_append(const stub_ctx* c, lc3stub_rec* r)
{
    r->ctx = c->id; r->dec = c->dec;
    pthread_mutex_lock(&g_mu);
    if (g_n == g_cap) {
        const int cap = g_cap ? 2 * g_cap : 256;
        lc3stub_rec* q = (lc3stub_rec*)realloc(g_log, sizeof(lc3stub_rec) * (size_t)cap);
        if (q) { g_log = q; g_cap = cap; }
    }
    if (g_n < g_cap) {
        if (g_cfg_on) cfg_put("{\"ctx\":%d,\"call\":\"%s\",\"rec\":%d}\n", c->id, stub_kind_names[r->kind], g_n);
        g_log[g_n++] = *r;
    }
    const int fail = g_fail == c->id;
    pthread_mutex_unlock(&g_mu);
    return fail;
}
static stub_ctx* stub_new(int dec, int n_streams, int channels)
{
    stub_ctx* c = (stub_ctx*)calloc(1, sizeof *c);
    if (!c) return NULL;
    c->dec = dec; c->n_streams = n_streams; c->channels = channels;
    pthread_mutex_lock(&g_mu); c->id = g_next_ctx++; pthread_mutex_unlock(&g_mu);
    return c;
}
static void words16(const uint16_t* w, size_t n, int64_t* o) { o[0] = w && n > 0 ? w[0] : -1; o[1] = w && n > 1 ? w[1] : -1; o[2] = w && n > 0 ? w[n - 1] : -1; }
static void words8(const uint8_t* w, size_t n, int64_t* o) { o[0] = w && n > 0 ? w[0] : -1; o[1] = w && n > 1 ? w[1] : -1; o[2] = w && n > 0 ? w[n - 1] : -1; }

int lc3hip_create(void** ctx, const lc3d_plan* plan, int n_streams, int device) { *ctx = stub_new(0, n_streams, plan->channels); return *ctx ? 0 : 1; }
int lc3hip_dec_create(void** ctx, const lc3d_plan* plan, const float* tmpl, int n_streams, int device) { *ctx = stub_new(1, n_streams, plan->channels); return *ctx ? 0 : 1; }
int lc3hip_destroy(void* ctx) { free(ctx); return 0; }
int lc3hip_dec_destroy(void* ctx) { free(ctx); return 0; }
int lc3hip_set_template(void* ctx, const float* tmpl) { return 0; }
/* one line of the second log for a configuration call: its named arguments (-1: the call has none such), then the entries it carries.  chans: the encoder's
 * entries first .. first + count - 1 (of an upload: chans[0] is entry `first`), dchans: the decoder's, both NULL: none */
static int stub_cfg(void* ctx, const char* call, int first, int count, int bw_only, int mode, int on_stream, int sync, const lc3d_chan* chans, const lc3d_dchan* dchans)
{
    const stub_ctx* c = (const stub_ctx*)ctx;
    pthread_mutex_lock(&g_mu);
    if (g_cfg_on) {
        cfg_put("{\"ctx\":%d,\"call\":\"%s\",\"first\":%d,\"count\":%d,\"bw_only\":%d,\"mode\":%d,\"on_stream\":%d,\"sync\":%d,\"entries\":[", c->id, call, first, count,
                bw_only, mode, on_stream, sync);
        for (int i = 0; i < count && (chans || dchans); i++) {
            if (chans) cfg_put("%s{\"nbytes\":%d,\"bitrate\":%d,\"bandwidth\":%d,\"bw_cut_bin\":%d,\"bw_index\":%d,\"reset_attack\":%d}", i ? "," : "", chans[i].nbytes,
                               chans[i].bitrate, chans[i].bandwidth, chans[i].bw_cut_bin, chans[i].bw_index, chans[i].reset_attack);
            else cfg_put("%s{\"nbytes\":%d,\"in_off\":%d}", i ? "," : "", dchans[i].nbytes, dchans[i].in_off);
        }
        cfg_put("]}\n");
    }
    pthread_mutex_unlock(&g_mu);
    return 0;
}
int lc3hip_upload_chans(void* ctx, const lc3d_chan* chans, int first, int count) { return stub_cfg(ctx, "upload_chans", first, count, -1, -1, 0, 1, chans, NULL); }
int lc3hip_upload_chans_async(void* ctx, const lc3d_chan* chans, int first, int count, void* hip_stream, int bw_only)
{
    return stub_cfg(ctx, "upload_chans_async", first, count, bw_only, -1, hip_stream != NULL, 0, chans, NULL);
}
int lc3hip_upload_enc_table(void* ctx, const lc3d_chan* tab, int n) { return 0; }
int lc3hip_dec_upload_chans(void* ctx, const lc3d_dchan* chans, int first, int count) { return stub_cfg(ctx, "dec_upload_chans", first, count, -1, -1, 0, 1, NULL, chans); }
int lc3hip_dec_upload_table(void* ctx, const lc3d_dchan* tab, int n) { return 0; }
/* (a download leaves the host's copy as it is: the stub has no device whose configuration could differ) */
int lc3hip_download_chans(void* ctx, lc3d_chan* chans) { return stub_cfg(ctx, "download_chans", -1, -1, -1, -1, 0, 1, NULL, NULL); }
int lc3hip_dec_download_chans(void* ctx, lc3d_dchan* chans) { return stub_cfg(ctx, "dec_download_chans", -1, -1, -1, -1, 0, 1, NULL, NULL); }
float lc3hip_last_ms(void* ctx) { return 0.0f; }
float lc3hip_dec_last_ms(void* ctx) { return 0.0f; }
/* no device: a probe or an egress call fails behind its checks.  With lc3stub_device_args(1) the two calls succeed instead (device 0, no stream, no tables), so that
 * a call gets as far as looking for its sibling library, of which the stub build has none (tests/test_sibling_missing_cpu.py) */
int lc3hip_dec_probe_args(void* ctx, int* device, const lc3d_plan** plan_dev, const lc3d_dchan** tab_dev, int* tab_n, void** stream)
{
    *device = 0; *plan_dev = NULL; *tab_dev = NULL; *tab_n = 0; *stream = NULL;
    return !g_device_args;
}
int lc3hip_stream_args(void* ctx, int want_stream, int* device, void** stream) { *device = 0; *stream = NULL; return !g_device_args; }
int lc3hip_set_input_ready(void* ctx, int ready) { return 0; }
int lc3hip_dec_set_input_ready(void* ctx, int ready) { return 0; }
static int stub_placement(void* ctx, const long long* offsets_dev, long long capacity)
{
    lc3stub_rec r; memset(&r, 0, sizeof r);
    r.kind = STUB_PLACEMENT; r.p[0] = (uint64_t)(uintptr_t)offsets_dev;
    r.a[0] = capacity; r.a[1] = r.a[2] = r.b[0] = r.b[1] = r.b[2] = -1;
    (void)stub_append((const stub_ctx*)ctx, &r);
    return capacity < 0;
}
int lc3hip_set_pcm_placement(void* ctx, const long long* offsets_dev, long long capacity) { return stub_placement(ctx, offsets_dev, capacity); }
int lc3hip_dec_set_pcm_placement(void* ctx, const long long* offsets_dev, long long capacity) { return stub_placement(ctx, offsets_dev, capacity); }
static int stub_counts(void* ctx, const int32_t* counts_dev)
{
    lc3stub_rec r; memset(&r, 0, sizeof r);
    r.kind = STUB_COUNTS; r.p[0] = (uint64_t)(uintptr_t)counts_dev;
    r.a[0] = r.a[1] = r.a[2] = r.b[0] = r.b[1] = r.b[2] = -1;
    (void)stub_append((const stub_ctx*)ctx, &r);
    return 0;
}
int lc3hip_set_frame_counts(void* ctx, const int32_t* counts_dev) { return stub_counts(ctx, counts_dev); }
int lc3hip_dec_set_frame_counts(void* ctx, const int32_t* counts_dev) { return stub_counts(ctx, counts_dev); }
int lc3hip_last_status(void* ctx, uint8_t* status_host, int n) { return 0; }
int lc3hip_last_records(void* ctx, float* rec_host, int max_words) { return 0; }
int lc3hip_work_buffer(void* ctx, int i, const char** name, void** ptr, size_t* bytes, int* elem) { return 1; }           /* no device buffers: the table is empty */
int lc3hip_dec_work_buffer(void* ctx, int i, const char** name, void** ptr, size_t* bytes, int* elem) { return 1; }
int lc3hip_test_fastmath(int kind, const float* x_host, float* y_host, long long n) { return 1; }

int lc3hip_encode(void* ctx, const void* pcm, int pcm_on_device, int bitdepth, int n_frames, void* out, int out_stride, int out_on_device, void* hip_stream,
                  int sync, void* trace_host, const uint16_t* fsz_host, const uint16_t* bw_host)
{
    const stub_ctx* c = (const stub_ctx*)ctx;
    lc3stub_rec r; memset(&r, 0, sizeof r);
    r.kind = STUB_ENCODE; r.n_frames = n_frames; r.stride = out_stride; r.fmt = bitdepth; r.on_device = pcm_on_device; r.sync = sync;
    r.p[0] = (uint64_t)(uintptr_t)pcm; r.p[1] = (uint64_t)(uintptr_t)out; r.hip_stream = (uint64_t)(uintptr_t)hip_stream;
    words16(fsz_host, (size_t)c->n_streams * n_frames, r.a); words16(bw_host, (size_t)c->n_streams * n_frames, r.b);
    return stub_append(c, &r);
}
/* the calls whose per-frame words are in device memory: one line of the second log each, what the host decided of them (stride: out_stride, in_stride or -1) */
static int stub_device_call(void* ctx, const char* call, int n_frames, int stride, int fmt, int has_a, int has_b, int lim, int clear_resets, long long capacity, int sync)
{
    pthread_mutex_lock(&g_mu);
    if (g_cfg_on) cfg_put("{\"ctx\":%d,\"call\":\"%s\",\"n_frames\":%d,\"stride\":%d,\"fmt\":%d,\"has_a\":%d,\"has_b\":%d,\"lim\":%d,\"clear_resets\":%d,\"capacity\":%lld,\"sync\":%d}\n",
                          ((const stub_ctx*)ctx)->id, call, n_frames, stride, fmt, has_a, has_b, lim, clear_resets, capacity, sync);
    pthread_mutex_unlock(&g_mu);
    return 0;
}
int lc3hip_encode_rates_device(void* ctx, const void* pcm, int bitdepth, int n_frames, void* out, int out_stride, const int32_t* rates_dev, const int32_t* bws_dev,
                               const lc3d_rate_rule* rule, int32_t* num_bytes_dev, uint8_t* flags_dev, int clear_resets, void* hip_stream, int sync)
{
    return stub_device_call(ctx, "encode_rates_device", n_frames, out_stride, bitdepth, rates_dev != NULL, bws_dev != NULL, rule->lim, clear_resets, -1, sync);
}
int lc3hip_encode_packed(void* ctx, const void* pcm, int bitdepth, int n_frames, const int32_t* rates_dev, const int32_t* bws_dev, const lc3d_rate_rule* rule,
                         int order, void* out, long long capacity, long long* offsets_dev, long long* total_dev, int32_t* num_bytes_dev, uint8_t* flags_dev,
                         int clear_resets, void* hip_stream, int sync)
{
    return stub_device_call(ctx, "encode_packed", n_frames, -1, bitdepth, rates_dev != NULL, bws_dev != NULL, rule->lim, clear_resets, capacity, sync);
}
int lc3hip_dec_decode(void* ctx, const void* frames, int frames_on_device, int in_stride, const uint8_t* bfi_flags_host, const uint16_t* sizes_host,
                      int sizes_max_nbytes, int n_frames, void* pcm, int pcm_on_device, int bps, uint8_t* status_host, void* hip_stream, int sync, void* trace_host)
{
    const stub_ctx* c = (const stub_ctx*)ctx;
    lc3stub_rec r; memset(&r, 0, sizeof r);
    r.kind = STUB_DECODE; r.n_frames = n_frames; r.stride = in_stride; r.fmt = bps; r.on_device = pcm_on_device; r.sync = sync;
    r.p[0] = (uint64_t)(uintptr_t)frames; r.p[1] = (uint64_t)(uintptr_t)pcm; r.p[2] = (uint64_t)(uintptr_t)status_host; r.p[3] = (uint64_t)(uintptr_t)bfi_flags_host;
    r.hip_stream = (uint64_t)(uintptr_t)hip_stream;
    words16(sizes_host, (size_t)c->n_streams * n_frames, r.a); words8(bfi_flags_host, (size_t)c->n_streams * n_frames, r.b);
    return stub_append(c, &r);
}
int lc3hip_dec_decode_dsizes(void* ctx, const void* frames, int in_stride, const int32_t* num_bytes_dev, const uint8_t* bfi_dev, int n_frames, void* pcm, int bps,
                             uint8_t* status_dev, void* hip_stream, int sync)
{
    return stub_device_call(ctx, "dec_decode_dsizes", n_frames, in_stride, bps, num_bytes_dev != NULL, bfi_dev != NULL, -1, -1, -1, sync);
}
int lc3hip_dec_decode_packed(void* ctx, const void* frames, long long capacity, const long long* offsets_dev, const int32_t* num_bytes_dev, int max_bytes,
                             const uint8_t* bfi_dev, int n_frames, void* pcm, int bps, uint8_t* status_dev, void* hip_stream, int sync)
{
    return stub_device_call(ctx, "dec_decode_packed", n_frames, -1, bps, num_bytes_dev != NULL, bfi_dev != NULL, max_bytes, -1, capacity, sync);
}

static size_t stub_state_bytes(const void* ctx) { const stub_ctx* c = (const stub_ctx*)ctx; return c ? (size_t)STUB_STATE_BYTES * c->n_streams * c->channels : 0; }
/* get: every byte is the context's number, so that a test sees which shard wrote which slice */
static int stub_state(void* ctx, int kind, void* host, size_t bytes)
{
    const stub_ctx* c = (const stub_ctx*)ctx;
    lc3stub_rec r; memset(&r, 0, sizeof r);
    r.kind = kind; r.p[0] = (uint64_t)(uintptr_t)host; r.bytes = bytes;
    r.a[0] = r.a[1] = r.a[2] = r.b[0] = r.b[1] = r.b[2] = -1;
    if (kind == STUB_SET_STATE && bytes) { r.a[0] = ((const uint8_t*)host)[0]; r.a[2] = ((const uint8_t*)host)[bytes - 1]; }
    const int fail = stub_append(c, &r);
    if (fail || bytes != stub_state_bytes(ctx)) return 1;
    if (kind == STUB_GET_STATE) memset(host, c->id, bytes);
    return 0;
}
size_t lc3hip_state_bytes(void* ctx) { return stub_state_bytes(ctx); }
int lc3hip_get_state(void* ctx, void* host, size_t bytes) { return stub_state(ctx, STUB_GET_STATE, host, bytes); }
int lc3hip_set_state(void* ctx, const void* host, size_t bytes) { return stub_state(ctx, STUB_SET_STATE, (void*)host, bytes); }
size_t lc3hip_dec_state_bytes(void* ctx) { return stub_state_bytes(ctx); }
int lc3hip_dec_get_state(void* ctx, void* host, size_t bytes) { return stub_state(ctx, STUB_GET_STATE, host, bytes); }
int lc3hip_dec_set_state(void* ctx, const void* host, size_t bytes) { return stub_state(ctx, STUB_SET_STATE, (void*)host, bytes); }
static int stub_wait(void* ctx)
{
    lc3stub_rec r; memset(&r, 0, sizeof r);
    r.kind = STUB_WAIT;
    return stub_append((const stub_ctx*)ctx, &r);
}
int lc3hip_wait(void* ctx) { return stub_wait(ctx); }
int lc3hip_dec_wait(void* ctx) { return stub_wait(ctx); }
/* a stream-lifecycle call: the line of a configuration call (first: the first listed stream, count: the entries of cfg, n x channels, or 0 without cfg), then
 * one with the list and the header words */
static int stub_stream_state(void* ctx, const char* call, int mode, const int* streams, int n, const lc3d_chan* cfg, const lc3d_dchan* dcfg, int blob_on_device,
                             const uint32_t* hdr, void* hip_stream, int sync)
{
    const stub_ctx* c = (const stub_ctx*)ctx;
    stub_cfg(ctx, call, streams[0], cfg || dcfg ? n * c->channels : 0, -1, mode, hip_stream != NULL, sync, cfg, dcfg);
    pthread_mutex_lock(&g_mu);
    if (g_cfg_on) {
        cfg_put("{\"ctx\":%d,\"call\":\"%s_list\",\"blob_on_device\":%d,\"hdr\":[%u,%u,%u,%u],\"streams\":[", c->id, call, blob_on_device, hdr[0], hdr[1], hdr[2], hdr[3]);
        for (int i = 0; i < n; i++) cfg_put("%s%d", i ? "," : "", streams[i]);
        cfg_put("]}\n");
    }
    pthread_mutex_unlock(&g_mu);
    return 0;
}
int lc3hip_stream_state(void* ctx, int mode, const int* streams, int n, const lc3d_chan* cfg, void* blob, int blob_on_device, const uint32_t* hdr, uint8_t* status,
                        void* hip_stream, int sync)
{
    return stub_stream_state(ctx, "stream_state", mode, streams, n, cfg, NULL, blob_on_device, hdr, hip_stream, sync);
}
int lc3hip_dec_stream_state(void* ctx, int mode, const int* streams, int n, const lc3d_dchan* cfg, void* blob, int blob_on_device, const uint32_t* hdr,
                            uint8_t* status, void* hip_stream, int sync)
{
    return stub_stream_state(ctx, "dec_stream_state", mode, streams, n, NULL, cfg, blob_on_device, hdr, hip_stream, sync);
}
