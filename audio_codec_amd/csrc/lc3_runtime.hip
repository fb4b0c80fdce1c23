/* lc3_runtime.hip -- the C-ABI device shim (lc3_shim.h): the host side of the gfx950 library.  Contexts, uploads, streams and events, and every launch of the
 * kernels in lc3_kernels.hip: lc3hip_* for the encoder (enc_launch: enc_one_wave or enc_pipelined, then enc_writer), lc3hip_dec_* for the
 * decoder (dec_decode: dec_stage, dec_plan, dec_parse, dec_chain, dec_tail).  No device code here: the kernels are declared in lc3_kernel_decls.h, and what a launch is sized by is in lc3_launch.h and lc3_plan.h.
 * Compiled once; the build-time diagnostic switches that act on host code (LC3_DUP, LC3D_SETS, DEC_SETS) are this file's. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <unistd.h>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "lc3_plan.h"
#include "lc3_shim.h"
#include "lc3_launch.h"
#include "lc3_kernel_decls.h"

/* The launch census (lc3_shim.h: lc3hip_launch_census_*; LC3PLUS_LAUNCH_CENSUS=<path>): which kernel entry points this process has launched, and how often.  Every
 * launch of this file goes through LC3_LAUNCH.  Off - the default - a launch reads one process-wide flag; on, it takes a lock (the sharded batches launch from one
 * host thread per shard) and counts under the kernel's host handle.  A handle's name is resolved when it is first seen: the handle of an extern "C" kernel is an
 * exported object of this library whose symbol is the kernel's name in the code object, so dladdr gives it; hipKernelNameRefByPtr is asked where dladdr has no answer.
 * With the environment switch (read once, when the library is loaded) the census is on from the start and its lines are appended to <path>, in one write, when the
 * library is unloaded or the process exits: no HIP call is made that late. */
struct census_entry { const void* fn; unsigned long long n; std::string name; };
static std::atomic<int> g_census_on{0};
static std::mutex g_census_mu;
static std::vector<census_entry> g_census;
static void census_note(const void* fn)
{
    std::lock_guard<std::mutex> lk(g_census_mu);
    for (census_entry& e : g_census) if (e.fn == fn) { e.n++; return; }
    Dl_info di; const char* nm = nullptr;
    if (dladdr(fn, &di) && di.dli_sname && di.dli_saddr == fn) nm = di.dli_sname;
    if (!nm) { nm = hipKernelNameRefByPtr(fn, (hipStream_t)0); (void)hipGetLastError(); }
    char buf[32];
    if (!nm || !*nm) { snprintf(buf, sizeof buf, "kernel@%p", fn); nm = buf; }
    g_census.push_back({fn, 1ull, std::string(nm)});
}
static std::string census_text()
{
    std::lock_guard<std::mutex> lk(g_census_mu);
    std::string t;
    for (const census_entry& e : g_census) if (e.n) t += e.name + " " + std::to_string(e.n) + "\n";
    return t;
}
#define LC3_LAUNCH(k, ...) do { auto k_ = (k); if (g_census_on.load(std::memory_order_relaxed)) census_note((const void*)k_); hipLaunchKernelGGL(k_, __VA_ARGS__); } while (0)
extern "C" void lc3hip_launch_census_enable(int on) { g_census_on.store(on != 0, std::memory_order_relaxed); }
extern "C" void lc3hip_launch_census_reset(void) { std::lock_guard<std::mutex> lk(g_census_mu); for (census_entry& e : g_census) e.n = 0; }
extern "C" size_t lc3hip_launch_census_read(char* buf, size_t cap)
{
    const std::string t = census_text();
    if (buf && cap) { const size_t m = t.size() < cap - 1 ? t.size() : cap - 1; memcpy(buf, t.data(), m); buf[m] = 0; }
    return t.size() + 1;
}
static struct census_env {
    std::string path;
    census_env() { const char* e = getenv("LC3PLUS_LAUNCH_CENSUS"); if (e && *e) { path = e; g_census_on.store(1, std::memory_order_relaxed); } }
    ~census_env()
    {
        if (path.empty()) return;
        const std::string t = census_text();
        const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_APPEND, 0644);
        if (fd < 0) return;
        if (!t.empty() && write(fd, t.data(), t.size()) < 0) {}
        close(fd);
    }
} g_census_env;      /* defined behind what its destructor reads: destroyed first */

#define LC3D_MAX_RUNS 16
#define PKS_SUMS(n) (((size_t)(n) + PKS_TILE - 1) / PKS_TILE)      /* packed output: tile sums of the scan over n frames */
#ifndef LC3D_SETS
#define LC3D_SETS 3                     /* sets of hand-over buffers under the input-ready promise: that many calls may be in flight */
#endif
#define LC3D_AHEAD_MAX_FRAMES 256     /* lc3hip_set_input_ready: calls of up to this many frames overlap with their predecessor */
#define LC3D_RUN_FRAMES 16            /* frames per run when consecutive calls do not overlap (measured, 4096 streams x 64 frames: 8: 58.1, 16: 64.9, 32: 62.8, 64: 58.6 Mframes/s) */
#define LC3D_RUN_FRAMES_READY 64      /* under the input-ready promise (calls overlap, a call's own pipeline matters less: 8: 62.4, 16: 70.1, 32: 72.6, 64: 73.0) */
/* The diagnostic switches (LC3PLUS_* environment variables), read ONCE per context in lc3hip_create / lc3hip_dec_create: no function-local statics, so two threads
 * that drive two batches never race on them, and a context's behaviour does not change under it. */
struct lc3hip_opts {
    int fused, no_split, streams5, run_frames, runs, ahead_max, rate_stream /* -1 rule, 0, 1 */, pre_runs, pitch2, scf_wave, front4, shape_fpw, shape_on_s, shape_wave,
        pack_wpg, pack_stream /* -1 off (default), 0, 1 */, resample48, resample96, dec_imdct4, check_ready, tailw_bytes, dec_parse_pad_kb, pack_pad_kb, pack_split, pack_w5, fuse_vq, stream_order, stream_skip, rate_on, dec_plc_stream, shape_on_pitch, side_prio, ragged_pipe,
        poison_work /* 0 off, 1 set A, 2 set B */, poison_calls;
};
static int env_int(const char* name, int lo, int hi, int dflt) { const char* e = getenv(name); if (!e || !*e) return dflt; const int v = atoi(e); return v >= lo && v <= hi ? v : dflt; }
static void read_opts(lc3hip_opts* o)
{
    o->fused = env_int("LC3PLUS_ENC_FUSED", 0, 1, 0);                 /* the bitstream writer inside lc3_encode_kernel */
    o->no_split = env_int("LC3PLUS_ENC_NO_SPLIT", 0, 1, 0);           /* everything in lc3_encode_kernel */
    o->streams5 = env_int("LC3PLUS_ENC_STREAMS", 0, 8, 0) >= 5;       /* the pitch kernel and the one-frame-per-lane kernels on streams of their own (GPU_MAX_HW_QUEUES >= 6) */
    o->run_frames = env_int("LC3PLUS_ENC_RUN_FRAMES", 1, 1 << 20, 0);
    o->runs = env_int("LC3PLUS_ENC_RUNS", 1, 16, 0);
    o->ahead_max = env_int("LC3PLUS_ENC_AHEAD_MAX", 1, 1 << 20, 0);
    o->rate_stream = env_int("LC3PLUS_ENC_RATE_STREAM", 0, 1, -1);
    o->pre_runs = env_int("LC3PLUS_ENC_PRE_RUNS", 1, 64, 3);
    o->pitch2 = env_int("LC3PLUS_ENC_PITCH2", 0, 1, 1);              /* 0 = one stream per wave */
    o->scf_wave = env_int("LC3PLUS_ENC_SCF_WAVE", 0, 1, 0);          /* energies / scale factors in the front kernel */
    o->front4 = env_int("LC3PLUS_ENC_FRONT4", 0, 1, 1);              /* 0 = the one-frame-at-a-time front for every frame length */
    o->shape_fpw = env_int("LC3PLUS_ENC_SHAPE_FPW", 1, 64, 0);
    o->shape_on_s = env_int("LC3PLUS_ENC_SHAPE_ON_S", 0, 1, 0);
    o->shape_wave = env_int("LC3PLUS_ENC_SHAPE_WAVE", 0, 1, 0);      /* the wave-per-frame shape kernel */
    o->pack_wpg = env_int("LC3PLUS_ENC_PACK_WPG", 1, 4, 4);          /* waves per workgroup of the writer */
    o->pack_stream = env_int("LC3PLUS_ENC_PACK_STREAM", 0, 1, -1);   /* 1 = the writers of consecutive calls on two side streams (deployment switch, see enc_writer) */
    o->resample48 = env_int("LC3PLUS_ENC_RESAMPLE48", 0, 1, 1);      /* 0 = the two-outputs-per-lane resampler for 48 kHz / 10 ms too */
    o->resample96 = env_int("LC3PLUS_ENC_RESAMPLE96", 0, 2, 1);      /* the four-outputs-per-lane resampler for 96 kHz: 0 never, 1 standard kernel layout (2.5 ms frames), 2 every frame length */
    /* frames of this size and more: tail + writer a frame per wave (lc3_enc_tailw_kernel).  Off (0) by default - measured, Mframes/s: c96 (320-byte frames) 32.5 without,
     * 27.3 with; c5 (20 ... 400 bytes) 86.5 without, 68.6 / 73.6 / 78.4 from 120 / 200 / 320 bytes: the wave-parallel writer shortens the longest wave of the call but
     * costs several times the instructions per frame, and the call is bound by instructions, not by that latency. */
    o->tailw_bytes = env_int("LC3PLUS_ENC_TAILW_BYTES", 0, 1 << 20, 0);
    o->dec_parse_pad_kb = env_int("LC3PLUS_DEC_PARSE_PAD_KB", 0, 60, -1);  /* LDS padding per parse workgroup = fewer resident parse waves; -1: the rule in dec_parse */
    o->pack_pad_kb = env_int("LC3PLUS_ENC_PACK_PAD_KB", 0, 60, -1);      /* LDS padding per writer workgroup = fewer resident writer waves; -1: the rule in enc_writer */
    o->pack_split = env_int("LC3PLUS_ENC_PACK_SPLIT", 0, 1, -1);        /* the writer as two kernels (head, coder); -1: the rule in enc_writer */
    o->pack_w5 = env_int("LC3PLUS_ENC_PACK_W5", 0, 1, -1);              /* the writer under a 96-register budget; -1: the rule in enc_writer (long calls of small 10 ms frames) */
    o->fuse_vq = env_int("LC3PLUS_ENC_FUSE_VQ", 0, 1, 0);               /* the SNS quantiser at the tail of the scale-factor kernel where no stream has attack handling */
    o->stream_order = env_int("LC3PLUS_ENC_STREAM_ORDER", 0, 1, 1);     /* diagnostic: 0 = the pitch stream is created before the front stream */
    o->stream_skip = env_int("LC3PLUS_ENC_STREAM_SKIP", 0, 8, 0);
    o->rate_on = env_int("LC3PLUS_ENC_RATE_ON", 0, 1, -1);                /* a rate chain that leaves the caller's stream runs on the front stream (0) / the pitch stream (1); -1: the rule in enc_pipelined */
    o->dec_plc_stream = env_int("LC3PLUS_DEC_PLC_STREAM", 0, 1, 1);        /* 0 = the decoder's concealment bookkeeping on the caller's stream (round 3) */
    o->shape_on_pitch = env_int("LC3PLUS_ENC_SHAPE_ON_PITCH", 0, 1, -1);  /* the shape kernel on the pitch stream; -1: the rule in enc_run (long calls of 2.5 ms high-resolution frames only) */
    o->side_prio = env_int("LC3PLUS_ENC_SIDE_PRIO", 0, 2, 0);             /* diagnostic: 1 = the side streams at the lowest HIP stream priority, 2 = at the highest */
    o->ragged_pipe = env_int("LC3PLUS_ENC_RAGGED_PIPE", 0, 1, 1);         /* 0 = every ragged encode call on the one-wave kernels, whatever its length (enc_launch: the A/B handle and a deployment's fallback) */
    o->check_ready = env_int("LC3PLUS_CHECK_READY", 0, 1, 0);        /* debug aid for lc3plus_enc_batch_set_input_ready: refuse a call made while foreign work is pending on the caller's stream */
    o->dec_imdct4 = env_int("LC3PLUS_DEC_IMDCT4", 0, 1, 1);          /* 0 = the one-frame-at-a-time IMDCT for N = 480 too */
    /* poisoned workspaces (work_poison_new, work_poison_all): A or B fills every work buffer with that set's typed poison where it is allocated; with
     * LC3PLUS_POISON_CALLS=1 every encode and decode call fills all of them again at its entry.  Debugging aids, off by default */
    { const char* e = getenv("LC3PLUS_POISON_WORK"); o->poison_work = e && (e[0] == 'A' || e[0] == 'B') && !e[1] ? 1 + (e[0] == 'B') : 0; }
    o->poison_calls = o->poison_work ? env_int("LC3PLUS_POISON_CALLS", 0, 1, 0) : 0;
}
/* The work buffers of a batch: the device buffers that a call fills and reads itself, and that no later call may rely on (DESIGN.md "Every workspace word").  One
 * table per context struct lists them (enc_work, dec_work): member, how many pointers the member holds, element type, and the bytes of pointer k as they follow from
 * the capacity the context keeps for it.  The poison routines and the two debug entries (lc3hip_work_buffer, lc3hip_dec_work_buffer) walk the table;
 * tests/test_poison_work_cpu.py holds it to the structs. */
struct work_buf { const char* name; size_t off; int n, elem; size_t (*bytes)(const void* ctx, int k); };
struct work_set { const void* ctx; const work_buf* tab; int n_tab, set /* lc3hip_opts.poison_work */, calls; };
#define WORK(T, member, n, elem, bytes_expr) {#member, offsetof(T, member), n, elem, [](const void* p_, int k) -> size_t { const T* c = (const T*)p_; (void)k; return (size_t)(bytes_expr); }}
/* What a batch keeps for those calls: the fresh-row template, and LC3D_SETS staging slots (pinned host memory for the index list, configuration entries and
 * host blobs, and its device copy) used in turn, each guarded by the event recorded behind the call that used it last; ev_done: behind the last call, for
 * later calls on other streams */
struct lc3hip_ss {
    float* d_tmpl; int row_words;
    uint8_t* h[LC3D_SETS]; uint8_t* d[LC3D_SETS]; size_t cap[LC3D_SETS]; hipEvent_t ev[LC3D_SETS]; int armed[LC3D_SETS], k;
    hipEvent_t ev_prev, ev_done; int done_armed;
};
/* Words of a call through pinned staging to the device, in LC3D_SETS rotating sets: the caller's array is free when the call returns, and a set is written again
 * once the call that read it has finished (calls with sync = 0) - its event is recorded by the caller behind the last kernel that reads the words. */
struct lc3hip_stage { uint16_t* d[LC3D_SETS]; uint16_t* h[LC3D_SETS]; size_t cap; hipEvent_t ev[LC3D_SETS]; int armed[LC3D_SETS], k; };
struct lc3hip_ctx {
    lc3hip_opts opt; work_set wk;
    int device, ncs, n_streams, channels, N, big, state_words, rs48, rs96;
    lc3d_plan* d_plan; lc3d_chan* d_chans; float* d_state;
    void* d_pcm; size_t pcm_cap; uint8_t* d_out; size_t out_cap;
    lc3d_trace* d_trace; size_t trace_cap;
    int* d_dumpv[LC3D_SETS]; size_t dump_capv[LC3D_SETS]; int hr, fused; float* d_y12[LC3D_SETS]; size_t y12_cap[LC3D_SETS];
    uint8_t* d_status; uint8_t* d_statusv[LC3D_SETS]; size_t status_capv[LC3D_SETS]; int status_frames;      /* d_status: the set of the last call */
    hipStream_t s_pk[2]; hipEvent_t ev_pk[2]; int pk_par;       /* the bitstream writers of consecutive calls beside each other (enc_writer) */
    float* d_spec[LC3D_SETS]; size_t spec_cap[LC3D_SETS]; float* d_frec[LC3D_SETS]; size_t frec_cap[LC3D_SETS]; hipEvent_t ev_done[LC3D_SETS]; float* d_xnext[LC3D_SETS + 1]; int xn_par, row_par; uint8_t* h_attack; int any_attack;
    const long long* plo; long long plcap;         /* lc3hip_set_pcm_placement: per-frame PCM offsets in device memory (null: off) and the buffer's length in elements */
    /* lc3hip_set_frame_counts: the caller's per-stream frame counts in device memory (null: off), and the clamped copy [n_streams] that the ragged plan kernel of a
     * call writes and its other kernels read.  One buffer: ragged calls are ordered on the caller's stream, none overlaps another.  rag: the call being queued is one - 1 with
     * per-frame bitrates, 2 without (its sizes are the carried ones: every frame of a stream has the bytes of the stream's configuration). */
    const int32_t* counts; int32_t* d_cnt; int rag;
    /* the index of the last run the previous pipelined call made (its ev_m / ev_f): what a call that overlaps it waits on; set with ahead_ok, read only while that is set */
    int ahead_last;
    int input_ready, ahead_ok, ahead_T, ahead_R;   /* lc3hip_set_input_ready: side kernels of a call beside the previous call's tail */   /* split path (lc3_enc_front.inc) */      /* per channel-frame status bits of the last call (LC3D_ENC_ST_*) */
    /* host-pointer pipeline (lc3hip_encode_host): two chunk slots, each with device staging and (for pageable callers) pinned staging */
    void* hp_dpcm[2]; void* hp_pin_in[2]; size_t hp_pcm_cap, hp_pin_in_cap;
    hipStream_t s_h2d; hipEvent_t ev_h2d[2], ev_k[2];
    hipStream_t s_pre, s_fr, s_pit, s_ln; hipEvent_t ev_rate; int rate_armed, mean_nbytes, min_nbytes, max_nbytes; int* h_nb; hipEvent_t ev_fork, ev_p[LC3D_MAX_RUNS], ev_f[LC3D_MAX_RUNS], ev_h[LC3D_MAX_RUNS], ev_m[LC3D_MAX_RUNS], ev_v[LC3D_MAX_RUNS];   /* side streams: pitch chain, frame-parallel front, frame-parallel tail */
    int ylen, srow, la, len12, fm_frames; const float* last_frec; int last_frec_frames;      /* the records of the last pipelined call (lc3hip_last_records) */
    hipStream_t stream, last_stream; hipEvent_t ev0, ev1; float last_ms;
    hipEvent_t ev_ours, ev_now; int ours_armed;       /* LC3PLUS_CHECK_READY: the tail of the library's own work on the caller's stream */
    /* per-frame bitrates: the configuration per channel byte count (lc3hip_upload_enc_table), and per call the stream-frame sizes, through pinned
     * staging, in LC3D_SETS rotating buffers (a buffer is written again once the call that read it has finished: calls with sync = 0) */
    lc3d_chan* d_etab; lc3hip_stage fsz;
    /* lc3hip_upload_chans_async: the configuration a per-frame-bitrate call leaves, queued on its stream behind its kernels from pinned staging; every later
     * call waits for the copy (ev_chans) on its own stream - and for the last stream-lifecycle call (lc3hip_stream_state), which records the same event */
    lc3d_chan* h_chans; hipEvent_t ev_chans; int chans_armed;
    /* per-frame bandwidths: per call the words in force, through pinned staging in LC3D_SETS rotating buffers as the sizes above.  The copy of a call goes on
     * the stream of the first kernel that reads the words (bw_to): on the pipelined path a side stream, so that a call that overlaps its predecessor does not
     * wait for that call's tail on the caller's stream; kernels on another stream wait for ev_bwcp.  bw_src / bw_bytes / bw_on: the pending call's copy. */
    int cfg_fresh;      /* a copy of lc3hip_upload_chans_async that the side streams are not yet ordered behind: 1 bandwidth words only, 2 more (enc_pipelined) */
    lc3hip_stage bw;
    const uint16_t* bw_src; size_t bw_bytes; hipStream_t bw_on; hipEvent_t ev_bwcp;
    lc3hip_ss ss;                                   /* lc3hip_set_template, lc3hip_stream_state */
    /* per-frame rates and bandwidths from device memory (lc3hip_encode_rates_device).  d_carry: each stream's rate, bytes and bandwidth in force, passed
     * from plan kernel to plan kernel in call order (ev_plan: behind the last one, on whichever stream it ran); carry_seed: the host has written the
     * configuration since, the next plan kernel starts from d_chans.  Per call, in LC3D_SETS rotating sets: the sizes and bandwidths the plan kernel writes
     * and the carry after the call (for the tail kernel); a set is written again behind the event of the call that used it last, waited for on the device.
     * pl: the plan kernel of the pending call, launched by bw_to where the first kernel that reads its words runs. */
    int4* d_carry; int carry_seed; hipEvent_t ev_plan, ev_pset_prev; int plan_armed;
    uint16_t* d_pfsz[LC3D_SETS]; uint16_t* d_pbw[LC3D_SETS]; int4* d_pend[LC3D_SETS]; size_t pset_frames; hipEvent_t ev_pset[LC3D_SETS]; int pset_armed[LC3D_SETS], pset;
    int etab_attack, etab_max;                      /* some byte count of the table has attack handling; the largest channel byte count */
    struct { int pending, k, T; const int32_t* rates; const int32_t* bws; int32_t* nb; uint8_t* fl; lc3d_rate_rule rule; int stride; } pl;
    /* packed output (lc3hip_encode_packed), for the call being queued: the scan (pack_scan) writes the table of offsets the writers read - per plan set k
     * with rates or bandwidths (a set is written again behind the call that used it last, as the plan buffers), one table otherwise (on the launch stream) */
    struct { int on, order; long long cap; long long* offs; long long* total; int32_t* nb; uint8_t* fl; const long long* tab; } pk;
    long long* d_poff[LC3D_SETS + 1]; size_t poff_cap /* frames; d_pbsum: a slot of PKS_SUMS(poff_cap) sums per table */; long long* d_pbsum; hipEvent_t ev_scan;
};

#define LC3D_FUSED_MAX_T 8
#define LC3D_FUSED_MAX_T_READY 5     /* measured under the promise (Mframes/s, pipelined / in-kernel writer): 4 frames 31.6 / 38, 6: 46.2 / 40, 8: 52.4 / 41 */
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "lc3plus_hip: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); return 1; } } while (0)
/* inside the create functions: release what has been allocated so far (the caller only sees ctx == NULL) */
#define HIPCHK_OR(x, cleanup) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "lc3plus_hip: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); cleanup; return 1; } } while (0)
/* waits for the call on s and keeps its kernel time (ev0 ... ev1) */
#define SYNC_TIMED(c, s) do { HIPCHK(hipStreamSynchronize(s)); float ms_ = 0; if (hipEventElapsedTime(&ms_, (c)->ev0, (c)->ev1) == hipSuccess) (c)->last_ms = ms_; } while (0)
static size_t ss_up(size_t x) { return (x + 255) & ~(size_t)255; }
/* the encoder's work buffers.  Not here: d_state, d_chans, d_carry, d_xnext and the lifecycle staging (a later call reads what an earlier one wrote), d_plan, d_etab and
 * the template (written once), d_status (points into d_statusv) */
static const work_buf enc_work[] = {
    WORK(lc3hip_ctx, d_pcm, 1, LC3HIP_ELEM_U8, c->pcm_cap),
    WORK(lc3hip_ctx, d_out, 1, LC3HIP_ELEM_U8, c->out_cap),
    WORK(lc3hip_ctx, d_trace, 1, LC3HIP_ELEM_U8, c->trace_cap),
    WORK(lc3hip_ctx, hp_dpcm, 2, LC3HIP_ELEM_U8, c->hp_pcm_cap),
    WORK(lc3hip_ctx, d_dumpv, LC3D_SETS, LC3HIP_ELEM_I32, c->dump_capv[k] * sizeof(int)),
    WORK(lc3hip_ctx, d_y12, LC3D_SETS, LC3HIP_ELEM_F32, c->y12_cap[k] * sizeof(float)),
    WORK(lc3hip_ctx, d_statusv, LC3D_SETS, LC3HIP_ELEM_U8, c->status_capv[k]),
    WORK(lc3hip_ctx, d_spec, LC3D_SETS, LC3HIP_ELEM_F32, c->spec_cap[k] * sizeof(float)),
    WORK(lc3hip_ctx, d_frec, LC3D_SETS, LC3HIP_ELEM_F32, c->frec_cap[k] * sizeof(float)),
    WORK(lc3hip_ctx, d_cnt, 1, LC3HIP_ELEM_I32, sizeof(int32_t) * (size_t)c->n_streams),
    WORK(lc3hip_ctx, fsz.d, LC3D_SETS, LC3HIP_ELEM_U16, c->fsz.cap),
    WORK(lc3hip_ctx, bw.d, LC3D_SETS, LC3HIP_ELEM_U16, c->bw.cap),
    WORK(lc3hip_ctx, d_pfsz, LC3D_SETS, LC3HIP_ELEM_U16, sizeof(uint16_t) * (size_t)c->n_streams * c->pset_frames),
    WORK(lc3hip_ctx, d_pbw, LC3D_SETS, LC3HIP_ELEM_U16, sizeof(uint16_t) * (size_t)c->n_streams * c->pset_frames),
    WORK(lc3hip_ctx, d_pend, LC3D_SETS, LC3HIP_ELEM_I32, sizeof(int4) * (size_t)c->n_streams),
    WORK(lc3hip_ctx, d_poff, LC3D_SETS + 1, LC3HIP_ELEM_I64, c->poff_cap * sizeof(long long)),
    WORK(lc3hip_ctx, d_pbsum, 1, LC3HIP_ELEM_I64, (LC3D_SETS + 1) * PKS_SUMS(c->poff_cap) * sizeof(long long)),
};
/* one buffer filled with the poison of its element type.  A stale word used as an index must stay tame, one used as a value must be wrong: set A is all ones (a
 * NaN, -1), set B small, finite and wrong (1.5f, 1) - a NaN can hide behind a comparison that is false or behind fmaxf; an int64 is an offset: -1 in both */
static int poison_fill(void* p, size_t bytes, int elem, int set)
{
    if (!p || !bytes) return 0;
    const bool a = set == 1;
    switch (elem) {
    case LC3HIP_ELEM_F32: HIPCHK(hipMemsetD32((hipDeviceptr_t)p, a ? -1 : 0x3FC00000 /* 1.5f */, bytes / 4)); break;
    case LC3HIP_ELEM_I32: HIPCHK(hipMemsetD32((hipDeviceptr_t)p, a ? -1 : 1, bytes / 4)); break;
    case LC3HIP_ELEM_U16: HIPCHK(hipMemsetD16((hipDeviceptr_t)p, a ? 0xFFFF : 1, bytes / 2)); break;
    case LC3HIP_ELEM_U8: HIPCHK(hipMemsetD8((hipDeviceptr_t)p, a ? 0xFF : 1, bytes)); break;
    case LC3HIP_ELEM_I64: HIPCHK(hipMemsetD8((hipDeviceptr_t)p, 0xFF, bytes)); break;
    default: return 1;
    }
    return 0;
}
/* LC3PLUS_POISON_WORK: the buffers grow_group has just allocated, those of them that the table lists.  The buffers are new - no call reads them - and the fill is
 * complete when this returns: a call that allocates never overlaps its predecessor, so the overlap under the input-ready promise is what it was */
struct lc3hip_buf;
static int work_poison_new(const work_set* wk, const lc3hip_buf* b, int n);
/* LC3PLUS_POISON_CALLS: every work buffer the batch holds, at the entry of a call.  Between two waits for the whole device: the calls before this one have
 * finished with the buffers, and no copy or kernel of this call starts before they are filled.  This SERIALISES consecutive calls, the promise's overlap
 * included - intended: it is the simple correct form (a fill threaded through the set-rotation events would be one more thing to get wrong).  A buffer the
 * call goes on to grow is poisoned where it is allocated, so every work buffer holds poison when the call's first copy or launch is queued. */
static int work_poison_all(const work_set* wk)
{
    HIPCHK(hipDeviceSynchronize());
    for (int e = 0; e < wk->n_tab; e++)
        for (int k = 0; k < wk->tab[e].n; k++)
            if (poison_fill(*(void* const*)((const char*)wk->ctx + wk->tab[e].off + k * sizeof(void*)), wk->tab[e].bytes(wk->ctx, k), wk->tab[e].elem, wk->set)) return 1;
    HIPCHK(hipDeviceSynchronize());
    return 0;
}
/* buffer i of the table in member order, for the two debug entries */
static int work_buffer_at(const work_set* wk, int i, const char** name, void** ptr, size_t* bytes, int* elem)
{
    static thread_local char label[64];
    for (int e = 0; e < wk->n_tab && i >= 0; i -= wk->tab[e++].n)
        if (i < wk->tab[e].n) {
            if (wk->tab[e].n > 1) snprintf(label, sizeof label, "%s[%d]", wk->tab[e].name, i); else snprintf(label, sizeof label, "%s", wk->tab[e].name);
            *name = label; *ptr = *(void* const*)((const char*)wk->ctx + wk->tab[e].off + i * sizeof(void*)); *elem = wk->tab[e].elem;
            *bytes = *ptr ? wk->tab[e].bytes(wk->ctx, i) : 0;
            return 0;
        }
    return 1;
}
/* The one place a buffer grows.  n buffers (device memory, or pinned host memory) share the capacity *cap, in the caller's unit: where it is below `need` they are
 * freed and allocated again, b[i].bytes each.  wait: an earlier call that did not wait may still read them - wait for the device before freeing, unless this is the
 * first allocation.  (hipFree drains the device too; the flag states where the order is the library's to keep.)  The pointers are null and the capacity is 0 before
 * anything is allocated, so a failed allocation leaves nothing in the context to write through or to free twice. */
struct lc3hip_buf { void** p; size_t bytes; bool pinned; };
static int grow_group(size_t* cap, size_t need, const lc3hip_buf* b, int n, bool wait, const work_set* wk = nullptr)
{
    if (*cap >= need) return 0;
    bool first = true;
    for (int i = 0; i < n; i++) first = first && !*b[i].p;
    if (wait && !first) HIPCHK(hipDeviceSynchronize());
    *cap = 0;
    for (int i = 0; i < n; i++) { void* old = *b[i].p; *b[i].p = nullptr; if (old) HIPCHK(b[i].pinned ? hipHostFree(old) : hipFree(old)); }
    for (int i = 0; i < n; i++) HIPCHK(b[i].pinned ? hipHostMalloc(b[i].p, b[i].bytes, hipHostMallocDefault) : hipMalloc(b[i].p, b[i].bytes));
    *cap = need;
    return wk && wk->set ? work_poison_new(wk, b, n) : 0;
}
static int work_poison_new(const work_set* wk, const lc3hip_buf* b, int n)
{
    for (int i = 0; i < n; i++) {
        const size_t at = (size_t)((const char*)b[i].p - (const char*)wk->ctx);
        for (int e = 0; e < wk->n_tab && !b[i].pinned; e++)
            if (at >= wk->tab[e].off && at < wk->tab[e].off + wk->tab[e].n * sizeof(void*) && poison_fill(*b[i].p, b[i].bytes, wk->tab[e].elem, wk->set)) return 1;
    }
    HIPCHK(hipDeviceSynchronize());
    return 0;
}
template <typename T> static int grow(T** p, size_t* cap, size_t need, size_t bytes, bool wait, const work_set* wk = nullptr) { const lc3hip_buf b = {(void**)p, bytes, false}; return grow_group(cap, need, &b, 1, wait, wk); }
/* two plain forms: grow_once, a buffer whose size never changes, allocated on first use (capacity 1 once it exists); replace, a buffer allocated anew whatever its size (capacity 0) */
template <typename T> static int grow_once(T** p, size_t bytes, bool pinned = false, const work_set* wk = nullptr) { size_t cap = *p != nullptr; const lc3hip_buf b = {(void**)p, bytes, pinned}; return grow_group(&cap, 1, &b, 1, false, wk); }
template <typename T> static int replace(T** p, size_t bytes) { size_t cap = 0; const lc3hip_buf b = {(void**)p, bytes, false}; return grow_group(&cap, 1, &b, 1, false); }
/* src into the set whose turn it is (returned in *set, armed); the copy h -> d is the caller's to queue.  Sized on first use, a call of equal or smaller size allocates nothing. */
static int stage_words(lc3hip_stage* q, const uint16_t* src, size_t bytes, int* set, const work_set* wk)
{
    const int k = q->k;
    if (q->armed[k]) HIPCHK(hipEventSynchronize(q->ev[k]));       /* the set of the call LC3D_SETS back */
    if (q->cap < bytes) {
        for (int i = 0; i < LC3D_SETS; i++) if (q->armed[i]) { HIPCHK(hipEventSynchronize(q->ev[i])); q->armed[i] = 0; }      /* no call reads them any more: no wait for the device */
        lc3hip_buf b[2 * LC3D_SETS];
        for (int i = 0; i < LC3D_SETS; i++) { b[2 * i] = {(void**)&q->d[i], bytes, false}; b[2 * i + 1] = {(void**)&q->h[i], bytes, true}; }
        if (grow_group(&q->cap, bytes, b, 2 * LC3D_SETS, false, wk)) return 1;
    }
    if (!q->ev[0]) for (int i = 0; i < LC3D_SETS; i++) HIPCHK(hipEventCreateWithFlags(&q->ev[i], hipEventDisableTiming));
    memcpy(q->h[k], src, bytes);
    q->armed[k] = 1; q->k = (k + 1) % LC3D_SETS; *set = k;
    return 0;
}
static void stage_free(lc3hip_stage* q) { for (int i = 0; i < LC3D_SETS; i++) { if (q->d[i]) hipFree(q->d[i]); if (q->h[i]) hipHostFree(q->h[i]); if (q->ev[i]) hipEventDestroy(q->ev[i]); } }
/* the template to the device, and every row of the batch reset from it (create) */
static int ss_init(lc3hip_ss* q, int device, float* state, int row_words, int ncs, const float* tmpl)
{
    HIPCHK(hipSetDevice(device));
    q->row_words = row_words;
    if (grow_once(&q->d_tmpl, sizeof(float) * (size_t)row_words)) return 1;
    HIPCHK(hipMemcpy(q->d_tmpl, tmpl, sizeof(float) * (size_t)row_words, hipMemcpyHostToDevice));
    LC3_LAUNCH(lc3_stream_state_kernel, dim3((unsigned)ncs), dim3(WAVE), 0, (hipStream_t)0, (int)LC3D_SS_RESET, state, row_words, 1, (const int*)nullptr, ncs,
                       (const float*)q->d_tmpl, (uint8_t*)nullptr, 0u, 0u, 0u, 0u, (uint8_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize((hipStream_t)0));
    return 0;
}
static void ss_free(lc3hip_ss* q)
{
    if (q->d_tmpl) hipFree(q->d_tmpl);
    for (int i = 0; i < LC3D_SETS; i++) { if (q->h[i]) hipHostFree(q->h[i]); if (q->d[i]) hipFree(q->d[i]); if (q->ev[i]) hipEventDestroy(q->ev[i]); }
    if (q->ev_prev) { hipEventDestroy(q->ev_prev); hipEventDestroy(q->ev_done); }
}
/* one lifecycle call on stream s, behind `last` (the stream of the batch's last call); cfg_bytes: bytes of one configuration entry */
static int ss_run(lc3hip_ss* q, hipStream_t s, hipStream_t last, int mode, float* state, int channels, const int* list, int n, const void* cfg, int cfg_bytes,
                  void* chans, void* blob, int blob_on_device, const uint32_t* hdr, uint8_t* status, int sync)
{
    if (!q->ev_prev) {
        HIPCHK(hipEventCreateWithFlags(&q->ev_prev, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&q->ev_done, hipEventDisableTiming));
        for (int i = 0; i < LC3D_SETS; i++) HIPCHK(hipEventCreateWithFlags(&q->ev[i], hipEventDisableTiming));
    }
    const size_t blob_bytes = (size_t)n * (LC3D_SS_HEADER + (size_t)channels * q->row_words * 4);
    const size_t o_cfg = ss_up(sizeof(int) * (size_t)n), n_cfg = cfg ? (size_t)n * channels * cfg_bytes : 0;
    const size_t o_blob = o_cfg + ss_up(n_cfg), need = o_blob + (blob_on_device ? 0 : blob_bytes);
    const int k = q->k;
    if (q->armed[k]) { HIPCHK(hipEventSynchronize(q->ev[k])); q->armed[k] = 0; }      /* the call LC3D_SETS back has read this slot */
    /* at least 64 KB; no wait for the device: the event above says the slot's last reader has finished */
    const size_t cap = need < (64u << 10) ? (64u << 10) : need;
    const lc3hip_buf b[] = {{(void**)&q->h[k], cap, true}, {(void**)&q->d[k], cap, false}};
    if (need && grow_group(&q->cap[k], cap, b, 2, false)) return 1;
    memcpy(q->h[k], list, sizeof(int) * (size_t)n);
    if (cfg) memcpy(q->h[k] + o_cfg, cfg, n_cfg);
    if (mode == LC3D_SS_IMPORT && !blob_on_device) memcpy(q->h[k] + o_blob, blob, blob_bytes);
    if (last && last != s) { HIPCHK(hipEventRecord(q->ev_prev, last)); HIPCHK(hipStreamWaitEvent(s, q->ev_prev, 0)); }
    HIPCHK(hipMemcpyAsync(q->d[k], q->h[k], mode == LC3D_SS_IMPORT && !blob_on_device ? o_blob + blob_bytes : o_blob, hipMemcpyHostToDevice, s));
    uint8_t* dblob = blob_on_device ? (uint8_t*)blob : q->d[k] + o_blob;
    LC3_LAUNCH(lc3_stream_state_kernel, dim3((unsigned)((size_t)n * channels)), dim3(WAVE), 0, s, mode, state, q->row_words, channels, (const int*)q->d[k], n,
                       (const float*)q->d_tmpl, dblob, hdr[0], hdr[1], hdr[2], hdr[3], blob_on_device ? status : (uint8_t*)nullptr,
                       (const uint32_t*)(cfg ? q->d[k] + o_cfg : nullptr), (uint32_t*)chans, cfg_bytes / 4);
    HIPCHK(hipGetLastError());
    if (mode == LC3D_SS_EXPORT && !blob_on_device) HIPCHK(hipMemcpyAsync(q->h[k] + o_blob, dblob, blob_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(q->ev[k], s)); q->armed[k] = 1; q->k = (k + 1) % LC3D_SETS;
    HIPCHK(hipEventRecord(q->ev_done, s)); q->done_armed = 1;
    if (mode == LC3D_SS_EXPORT && !blob_on_device) { HIPCHK(hipStreamSynchronize(s)); memcpy(blob, q->h[k] + o_blob, blob_bytes); }
    else if (sync) HIPCHK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int lc3hip_test_fastmath(int kind, const float* x_host, float* y_host, long long n)
{
    float *dx = nullptr, *dy = nullptr;
    HIPCHK(hipMalloc((void**)&dx, (size_t)n * 4)); HIPCHK(hipMalloc((void**)&dy, (size_t)n * 4));
    HIPCHK(hipMemcpy(dx, x_host, (size_t)n * 4, hipMemcpyHostToDevice));
    LC3_LAUNCH(lc3_fastmath_test_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, kind, dx, dy, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(y_host, dy, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipFree(dx)); HIPCHK(hipFree(dy));
    return 0;
}
extern "C" int lc3hip_destroy(void* ctx);
extern "C" int lc3hip_create(void** out_ctx, const lc3d_plan* plan, int n_streams, int device)
{
    int ndev = 0;
    *out_ctx = nullptr;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { fprintf(stderr, "lc3plus_hip: no HIP device available (this engine has no CPU fallback)\n"); return 1; }
    lc3hip_ctx* c = (lc3hip_ctx*)calloc(1, sizeof *c);
    if (!c) return 1;
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    c->device = device;
    HIPCHK_OR(hipSetDevice(device), free(c));
    c->n_streams = n_streams; c->channels = plan->channels; c->ncs = n_streams * plan->channels; c->N = plan->N;
    c->big = LC3D_LAYOUT_BIG(plan->N, plan->la);
    c->hr = plan->hrmode; c->ylen = plan->ylen; c->la = plan->la; c->len12 = plan->len12;
    c->fm_frames = (!c->big && plan->pfa_nst >= 2 && plan->pfa_rad[0] <= 8 && plan->pfa_rad[1] <= 8 && (plan->pfa_nst < 3 || plan->pfa_rad[2] <= 8) && plan->N <= 240) ? (plan->N > 120 ? FM_F240 : 8) : 0;      /* lc3_enc_frontm_kernel */
    c->srow = LC3D_SROW(plan->ylen);
    c->rs48 = plan->N == 480 && plan->rs_stride == 4 && plan->n12 == 128 && plan->rs_mem_in_len == 60;      /* lc3_enc_resample48_kernel */
    read_opts(&c->opt);
    if (!c->opt.resample48) c->rs48 = 0;
    /* lc3_enc_resample96_kernel_n*: 96 kHz.  By default for the standard kernel layout only (2.5 ms frames): c4 125.0 -> 137.0 Mframes/s; beside the large-layout kernels its
     * 256 registers per wave cost more than its shorter run gives (c96 36.6 -> 33.4) */
    c->rs96 = c->opt.resample96 && plan->rs_stride == 2 && plan->rs_mem_in_len == 120 && (plan->N == 960 || plan->N == 480 || plan->N == 240) && plan->n12 * 15 == plan->N * 2
              && (!c->big || c->opt.resample96 == 2);
    c->fused = c->opt.fused;
    c->state_words = LC3D_STATE_WORDS(c->big ? LC3D_MEMCAP_BIG : LC3D_MEMCAP_STD);
    HIPCHK_OR(hipMalloc((void**)&c->d_plan, sizeof(lc3d_plan)), lc3hip_destroy(c));
    HIPCHK_OR(hipMemcpy(c->d_plan, plan, sizeof(lc3d_plan), hipMemcpyHostToDevice), lc3hip_destroy(c));
    HIPCHK_OR(hipMalloc((void**)&c->d_chans, sizeof(lc3d_chan) * c->ncs), lc3hip_destroy(c));
    HIPCHK_OR(hipMalloc((void**)&c->d_state, sizeof(float) * c->state_words * (size_t)c->ncs), lc3hip_destroy(c));
    HIPCHK_OR(hipMalloc((void**)&c->d_cnt, sizeof(int32_t) * (size_t)n_streams), lc3hip_destroy(c));
    c->wk = {c, enc_work, (int)(sizeof enc_work / sizeof *enc_work), c->opt.poison_work, c->opt.poison_calls};
    if (c->wk.set && work_poison_all(&c->wk)) { lc3hip_destroy(c); return 1; }      /* what exists by now: the counts */
    /* the library's own launch stream is created when a call first needs it (a caller that brings its stream never does): HIP maps streams
     * onto a few hardware queues, and the pipelined path wants its three side streams on queues of their own */
    HIPCHK_OR(hipEventCreate(&c->ev0), lc3hip_destroy(c)); HIPCHK_OR(hipEventCreate(&c->ev1), lc3hip_destroy(c));
    *out_ctx = c;
    return 0;
}

extern "C" int lc3hip_stream_args(void* ctx, int want_stream, int* device, void** stream)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    if (!c) return 1;
    if (want_stream && !c->stream) { HIPCHK(hipSetDevice(c->device)); HIPCHK(hipStreamCreate(&c->stream)); }
    *device = c->device; *stream = (void*)c->stream;
    return 0;
}

extern "C" int lc3hip_set_template(void* ctx, const float* tmpl)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    if (ss_init(&c->ss, c->device, c->d_state, c->state_words, c->ncs, tmpl)) return 1;
    c->ahead_ok = 0;                       /* the MDCT memory is in the state again, not in the hand-over of a previous call */
    return 0;
}

static int chans_host_side(lc3hip_ctx* c, const lc3d_chan* chans, int first, int count);
extern "C" int lc3hip_upload_chans_async(void* ctx, const lc3d_chan* chans, int first, int count, void* hip_stream, int bw_only)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    c->cfg_fresh = bw_only ? 1 : 2;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (grow_once(&c->h_chans, sizeof(lc3d_chan) * (size_t)c->ncs, true)) return 1;
    if (!c->ev_chans) HIPCHK(hipEventCreateWithFlags(&c->ev_chans, hipEventDisableTiming));
    if (c->chans_armed) HIPCHK(hipEventSynchronize(c->ev_chans));      /* the staging of the previous copy is free */
    memcpy(c->h_chans + first, chans, sizeof(lc3d_chan) * (size_t)count);
    HIPCHK(hipMemcpyAsync(c->d_chans + first, c->h_chans + first, sizeof(lc3d_chan) * (size_t)count, hipMemcpyHostToDevice, s));
    c->carry_seed = 1;
    HIPCHK(hipEventRecord(c->ev_chans, s)); c->chans_armed = 1;
    if (c->opt.check_ready && c->ev_ours) { HIPCHK(hipEventRecord(c->ev_ours, s)); c->ours_armed = 1; }      /* the copy is the library's own work */
    return chans_host_side(c, chans, first, count);
}
extern "C" int lc3hip_upload_chans(void* ctx, const lc3d_chan* chans, int first, int count)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    /* a launch with sync = 0 may still be reading d_chans, possibly on a caller's non-blocking stream that a plain hipMemcpy does not
     * wait for: drain the stream the last launch went to first */
    if (c->last_stream) { HIPCHK(hipStreamSynchronize(c->last_stream)); c->last_stream = nullptr; }
    if (c->chans_armed) HIPCHK(hipEventSynchronize(c->ev_chans));      /* a queued copy of lc3hip_upload_chans_async lands first */
    HIPCHK(hipMemcpy(c->d_chans + first, chans, sizeof(lc3d_chan) * count, hipMemcpyHostToDevice));
    c->carry_seed = 1;
    return chans_host_side(c, chans, first, count);
}
/* what the launch decisions read of the configuration, on the host: channel-streams first ... first + count - 1, or with list the channels of streams list[0 .. count / channels - 1] */
static int chans_host_side_list(lc3hip_ctx* c, const lc3d_chan* chans, int first, int count, const int* list)
{
    if (!c->h_attack) { c->h_attack = (uint8_t*)calloc((size_t)c->ncs, 1); if (!c->h_attack) return 1; }
    if (!c->h_nb) { c->h_nb = (int*)calloc((size_t)c->ncs, sizeof(int)); if (!c->h_nb) return 1; }
    for (int i = 0; i < count; i++) {
        const int cs = list ? list[i / c->channels] * c->channels + i % c->channels : first + i;
        c->h_attack[cs] = chans[i].attack_handling != 0 || chans[i].reset_attack != 0;     /* streams with attack handling need lc3_enc_attack_kernel; a pending reset too */
        c->h_nb[cs] = chans[i].nbytes;
    }
    c->any_attack = 0;
    for (int i = 0; i < c->ncs; i++) c->any_attack |= c->h_attack[i];
    /* mean frame size: decides where the rate chain runs (enc_pipelined) */
    { long long sum = 0; int mn = 1 << 30, mx = 0; for (int i = 0; i < c->ncs; i++) { sum += c->h_nb[i]; if (c->h_nb[i] < mn) mn = c->h_nb[i]; if (c->h_nb[i] > mx) mx = c->h_nb[i]; }
      c->mean_nbytes = (int)(sum / (c->ncs > 0 ? c->ncs : 1)); c->min_nbytes = mn; c->max_nbytes = mx; }
    return 0;
}
static int chans_host_side(lc3hip_ctx* c, const lc3d_chan* chans, int first, int count) { return chans_host_side_list(c, chans, first, count, nullptr); }

/* the kernels of one call (or of one run of frames of a call) on stream s, PCM and output in device memory.  n_frames frames from
 * dpcm [stream][n_frames][channel][N]; the hand-over records and status bytes are rows of dT frames per channel-stream in which this
 * launch fills frames dt0 ... dt0 + n_frames - 1; with `pack` the bitstream writer then runs over all dT frames into dout [stream][dT][out_stride]. */
#ifdef LC3_DUP
/* diagnostic build (tools/variants.sh dup "-DLC3_DUP", tools/dup_run.sh): LC3PLUS_ENC_DUP=<letters> launches the named kernels of the pipelined
 * path twice (r resampler, h HP50, p pitch, f front, v quantiser, s rate, k pack) - what a kernel costs in the co-resident mix.  Output is
 * wrong for the kernels that carry state (h, p, s); never built into the product library. */
static int dup_of(char k) { static const char* e = nullptr; static bool rd = false; if (!rd) { e = getenv("LC3PLUS_ENC_DUP"); rd = true; } return e && strchr(e, k) ? 2 : 1; }
#define DUPL(k) for (int dup_ = 0; dup_ < dup_of(k); dup_++)
#else
#define DUPL(k)
#endif
/* How a launch picks its twin.  Every step of a path is launched at ONE place: a generic lambda that holds the grid, the stream and the
 * step's dense argument list, and takes the kernel and that kernel's trailing arguments - `go(kernel, trailing ...)`.  The variant is chosen beside it: the
 * kernel's name (plain, _fmt, _wire, _big, _w5, _l32 ...) by a conditional, a twin with more parameters (_plc: LC3_PLACED_ARGS, _rag: LC3_RAGGED_ARGS, _pk, _vbw)
 * by a call of the same lambda with those values appended.  The declaration of lc3_kernel_decls.h checks count and types of what arrives. */
/* the twin of `name` by sample type: the reference's three depths, the wire types, the other formats */
#define BY_FMT(q, name) ((q)->fmt_plain ? name : (q)->fmt_wire ? name##_wire : name##_fmt)
#define BY_FMT_RAG(q, name) ((q)->fmt_plain ? name##_rag : (q)->fmt_wire ? name##_wire_rag : name##_fmt_rag)      /* the ragged forms of the pipelined path */
/* PCM for the kernels that declare it as a typed pointer (the specialised resamplers): converts to whichever sample type the chosen kernel takes */
struct pcm_as { const void* p; template <typename T> operator const T*() const { return (const T*)p; } };
/* Placed PCM, calls that report per frame in device memory: behind the call's own kernels on s - every one of them that writes `out` (the encoder's flags, the
 * decoder's status) has finished or is joined to s by then - the frames whose offset is invalid get `bit`.  Nothing to do without placement or without `out`. */
static int placed_mark(const long long* plo, long long plcap, int channels, int N, long long n, uint8_t* out, int bit, hipStream_t s)
{
    if (!plo || !out || n <= 0) return 0;
    LC3_LAUNCH(lc3_pcm_placed_mark_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, plo, plcap, channels, N, n, out, bit);
    HIPCHK(hipGetLastError());
    return 0;
}
/* the 12.8 kHz polyphase FIR of frames hb ... hb + hn - 1 of every channel-stream on stream st: four outputs per lane where the shape allows */
static void launch_resample(lc3hip_ctx* c, hipStream_t st, const void* dpcm, int bitdepth, int n_frames, int hb, int hn, int mc, float* dy12, const float* xprev, int xprev_stride,
                            const int32_t* cnt = nullptr /* a ragged call: always the resampler for every shape, in its _rag form */)
{
    const unsigned pruns = (unsigned)((hn + PRE_FPW - 1) / PRE_FPW);
    const bool a16 = (((size_t)dpcm) & 15) == 0;
    /* the resampler for every shape, and its twins by sample type */
    auto any = [&](auto k, auto... placed) { LC3_LAUNCH(k, dim3((unsigned)c->ncs * pruns), dim3(WAVE), 0, st, c->d_plan, c->d_state, c->state_words, mc, dpcm, bitdepth, n_frames, hb, hn, c->ncs, dy12, xprev, xprev_stride, placed...); };
    /* the specialised ones take typed dense pointers: 16-bit samples ... */
    auto s16 = [&](auto k, unsigned runs) { LC3_LAUNCH(k, dim3((unsigned)c->ncs * runs), dim3(WAVE), 0, st, c->d_plan, (const int16_t*)dpcm, c->channels, mc, n_frames, hb, hn, c->ncs, dy12, xprev, xprev_stride); };
    /* ... and float32 or wire samples, which also take the format word */
    auto typed = [&](auto k) { LC3_LAUNCH(k, dim3((unsigned)c->ncs * pruns), dim3(WAVE), 0, st, c->d_plan, pcm_as{dpcm}, bitdepth, c->channels, mc, n_frames, hb, hn, c->ncs, dy12, xprev, xprev_stride); };
    if (cnt) {
        if (c->plo) any(lc3_enc_resample_plc_kernel_rag, c->plo, c->plcap, cnt);
        else any((bitdepth == 16 || bitdepth == 24 || bitdepth == 32) ? lc3_enc_resample_kernel_rag : lc3d_pcm_type_wire(bitdepth & LC3D_PCM_TYPE_MASK) ? lc3_enc_resample_wire_kernel_rag : lc3_enc_resample_fmt_kernel_rag, cnt);
    }
    else if (c->plo) any(lc3_enc_resample_plc_kernel, c->plo, c->plcap);      /* placed PCM: the resampler for every shape (the specialised ones take typed dense pointers) */
    else if (c->rs48 && bitdepth == 16 && a16) s16(lc3_enc_resample48_kernel, pruns);
    else if (c->rs48 && (bitdepth & (LC3D_PCM_TYPE_MASK | LC3D_PCM_INTERLEAVED)) == LC3D_PCM_FLOAT32 && a16) typed(lc3_enc_resample48f_kernel);   /* frames of 480 x 4 bytes: every one 16-byte aligned */
    else if (c->rs48 && lc3d_pcm_type_wire(bitdepth & LC3D_PCM_TYPE_MASK) && !(bitdepth & LC3D_PCM_INTERLEAVED) && (((size_t)dpcm) & 3) == 0) typed(lc3_enc_resample48w_kernel);   /* wire samples that follow each other, frames of 480 elements: every one starts on a dword */
    else if (c->rs96 && bitdepth == 16 && a16) {
        const int fpb = (1920 / c->N) * PRE96_ITERS;                       /* frames per workgroup: PRE96_ITERS steps of 1 920 samples */
        s16(c->N == 960 ? lc3_enc_resample96_kernel_n960 : c->N == 480 ? lc3_enc_resample96_kernel_n480 : lc3_enc_resample96_kernel_n240, (unsigned)((hn + fpb - 1) / fpb));
    }
    else any((bitdepth == 16 || bitdepth == 24 || bitdepth == 32) ? lc3_enc_resample_kernel : lc3d_pcm_type_wire(bitdepth & LC3D_PCM_TYPE_MASK) ? lc3_enc_resample_wire_kernel : lc3_enc_resample_fmt_kernel);
}
/* behind it the HP50 recurrence of the same frames, one stream per lane */
static void launch_hp50(lc3hip_ctx* c, hipStream_t st, int n_frames, int hb, int hn, int mc, float* dy12, const int32_t* cnt = nullptr)
{
    auto hp = [&](auto k, auto... ragged) { LC3_LAUNCH(k, dim3((unsigned)((c->ncs + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, c->d_plan, c->d_state, c->state_words, LC3D_ST_SCAL(mc), n_frames, hb, hn, c->ncs, dy12, ragged...); };
    if (cnt) hp(lc3_enc_hp50_kernel_rag, cnt); else hp(lc3_enc_hp50_kernel);
}
static int bw_to(lc3hip_ctx* c, hipStream_t st);
/* what enc_one_wave passes for the optional argument groups of the one-wave kernels (lc3_kernel_decls.h: LC3_OW_OPT orders them) */
#define LC3_OW_VALS_VAR_0
#define LC3_OW_VALS_VAR_1 , q->dfsz, (const lc3d_chan*)c->d_etab
#define LC3_OW_VALS_VBW_0
#define LC3_OW_VALS_VBW_1 , q->dbw
#define LC3_OW_VALS_PK_0
#define LC3_OW_VALS_PK_1 , pt
#define OW_KEY(big, var, vbw, pk) ((big) | (var) << 1 | (vbw) << 2 | (pk) << 3)
/* one call of enc_launch: its arguments, and what the functions it is cut into hand to each other */
struct enc_call {
    const void* dpcm; int bitdepth, n_frames; uint8_t* dout; int out_stride; hipStream_t s; lc3d_trace* dtr; int dT, dt0; bool pack;
    const uint16_t* dfsz;       /* per-frame bitrates: [stream][dT] stream-frame bytes, or null */
    const uint16_t* dbw;        /* per-frame bandwidths: [stream][dT] Hz in force (stage_bw), or null; the path is the one without them */
    bool fmt_plain, fmt_wire, placed;       /* which twin by sample type */
    const int32_t* cnt;         /* a ragged call: [stream] clamped frame counts, or null */
    bool rag_pipe;              /* ... on the pipelined path (the _rag form of every step); else the one-wave path with the _rag twins, no pre-kernels (enc_launch decides) */
    int set, mc, dstride; int* ddump; float* dy12; bool split;      /* enc_size_set: the call's set of hand-over buffers, and the path they select */
    bool rate_on_side;                      /* enc_pipelined: the rate chain left the caller's stream */
};
/* the call's set of hand-over buffers (rows, records, writer scratch, status bytes), sized.  No site here waits for the device itself: under the input-ready
 * promise every set is sized by the first call that needs it, and without it hipFree waits for the device's pending work before it releases a buffer that a
 * call with sync = 0 may still read. */
static int enc_size_set(lc3hip_ctx* c, enc_call* q, bool in_kernel_writer)
{
    const int set = q->set;
    /* under the input-ready promise every set is sized on the first call that needs it: no allocation inside a later (timed, overlapped) call */
    const int i0 = c->input_ready ? 0 : set, i1 = c->input_ready ? LC3D_SETS : set + 1;
    if (!in_kernel_writer) {
        q->dstride = PK_STRIDE(c->N, c->hr);
        const size_t need = (size_t)c->ncs * q->dT * q->dstride;
        for (int i = i0; i < i1; i++) if (grow(&c->d_dumpv[i], &c->dump_capv[i], need, need * sizeof(int), false, &c->wk)) return 1;
        q->ddump = c->d_dumpv[set];
    }
    /* ahead of it: the 12.8 kHz resampler of all frames at once and its HP50 recurrence one stream per lane (lc3_enc_pre.inc) */
    if (!q->dtr && !c->fused && (!q->cnt || q->rag_pipe)) {      /* (a ragged call on the one-wave path resamples in its one kernel, as a traced one: the dense pre-kernels read every frame's PCM) */
        const size_t need = (size_t)c->ncs * q->n_frames * 128;
        /* two buffers under the input-ready promise: the next call's resampler may run beside this call's pitch kernel */
        for (int i = i0; i < i1; i++) if (grow(&c->d_y12[i], &c->y12_cap[i], need, need * sizeof(float), false, &c->wk)) return 1;
        q->dy12 = c->d_y12[set];
    }
    q->split = q->dy12 && q->ddump && !c->opt.no_split;
    if (q->dt0 == 0) {   /* per channel-frame status bits (LC3D_ENC_ST_*), cleared per call: by the stream that runs the kernel that sets them (the writer's, on the pipelined path) */
        const size_t need = (size_t)c->ncs * q->dT;
        for (int i = i0; i < i1; i++) if (grow(&c->d_statusv[i], &c->status_capv[i], need, need, false, &c->wk)) return 1;
        c->d_status = c->d_statusv[set];
        if (!q->split) HIPCHK(hipMemsetAsync(c->d_status, 0, need, q->s));
        c->status_frames = q->dT;
    }
    if (q->split) {
        /* spectrum rows and records of all dT frames of the call (a call through host pointers comes in pieces: rows dt0 ...): two sets under
         * the input-ready promise (consecutive calls overlap: the side kernels of a call write one set while the bitstream writer of the call
         * before still reads the other), one otherwise */
        const size_t ns = (size_t)c->ncs * q->dT * c->srow, nr = (size_t)c->ncs * q->dT * FR_WORDS;
        for (int i = i0; i < i1; i++) {
            const size_t had = c->frec_cap[i];
            if (grow(&c->d_spec[i], &c->spec_cap[i], ns, ns * sizeof(float), false, &c->wk) || grow(&c->d_frec[i], &c->frec_cap[i], nr, nr * sizeof(float), false, &c->wk)) return 1;
            /* new records start as zeros, on s in front of the fork (a call that allocates never overlaps its predecessor): a record has padding words that no kernel
             * writes, and lc3hip_last_records reports the same words for the same call on two batches.  (No kernel reads them either: under LC3PLUS_POISON_WORK they
             * keep the poison, which two batches share as they share the zeros.) */
            if (c->frec_cap[i] != had && !c->wk.set) HIPCHK(hipMemsetAsync(c->d_frec[i], 0, nr * sizeof(float), q->s));
        }
        for (int i = 0; i < LC3D_SETS + 1; i++) if (grow_once(&c->d_xnext[i], (size_t)c->ncs * q->mc * sizeof(float))) return 1;
    }
    return 0;
}
/* everything in lc3_encode_kernel (traced, diagnostic and very short launches), behind the 12.8 kHz pre-kernels when they apply */
static int enc_one_wave(lc3hip_ctx* c, const enc_call* q)
{
    hipStream_t s = q->s;
    if (c->big && q->dbw) return 1;                          /* no such kernel (LC3_OW_KERNELS) */
    c->ahead_ok = 0; c->last_frec = nullptr; c->last_frec_frames = 0; c->cfg_fresh = 0;
    if (q->dy12) {
        launch_resample(c, s, q->dpcm, q->bitdepth, q->n_frames, 0, q->n_frames, q->mc, q->dy12, c->d_state + LC3D_ST_XPREV, c->state_words);
        launch_hp50(c, s, q->n_frames, 0, q->n_frames, q->mc, q->dy12);
        HIPCHK(hipGetLastError());
    }
    if (q->dbw && bw_to(c, s)) return 1;
    /* the one-wave kernel of this call by layout and optional argument groups (lc3_kernel_decls.h: LC3_OW_KERNELS), or its _fmt, _wire or _plc twin */
    const long long* pt = c->pk.on || q->cnt ? c->pk.tab : nullptr;         /* packed output: the _pk kernels, frames at the offsets of the call's table (a ragged call always has one) */
    const int key = OW_KEY(c->big != 0, q->dfsz != nullptr, q->dbw != nullptr, pt != nullptr);
    auto ow = [&](auto k, auto... groups) { LC3_LAUNCH(k, dim3(c->ncs), dim3(WAVE), 0, s, c->d_plan, c->d_chans, c->d_state, q->dpcm, q->bitdepth, q->n_frames, q->dout, pt ? 0 : q->out_stride, c->ncs, q->dtr, q->ddump, q->dstride, q->dy12, c->d_status, q->dT, q->dt0, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, groups...); };
#define OW_LAUNCH(name, big, var, vbw, pk) \
    if (key == OW_KEY(big, var, vbw, pk)) { \
        if (q->placed) ow(name##_plc LC3_OW_OPT(LC3_OW_VALS_, var, vbw, pk), c->plo, c->plcap); \
        else ow(BY_FMT(q, name) LC3_OW_OPT(LC3_OW_VALS_, var, vbw, pk)); \
    } else
#define OW_LAUNCH_RAG(name, big, var, vbw, pk) \
    if (key == OW_KEY(big, var, vbw, pk)) { \
        if (q->placed) ow(name##_rag_plc LC3_OW_OPT(LC3_OW_VALS_, var, vbw, pk), c->plo, c->plcap, q->cnt); \
        else ow((q->fmt_plain ? name##_rag : q->fmt_wire ? name##_rag_wire : name##_rag_fmt) LC3_OW_OPT(LC3_OW_VALS_, var, vbw, pk), q->cnt); \
    } else
    if (q->cnt) { LC3_OW_RAG_KERNELS(OW_LAUNCH_RAG) return 1; }      /* ragged: per-frame sizes and a table, or no such kernel */
    else LC3_OW_KERNELS(OW_LAUNCH) return 1;
#undef OW_LAUNCH_RAG
#undef OW_LAUNCH
    return 0;
}
/* the side streams of the pipelined path and their events, created on first use */
static int enc_side_streams(lc3hip_ctx* c)
{
    if (c->s_pre) return 0;
    /* Two side streams, no third.  HIP (four hardware queues by default) gave the FIRST side stream a batch creates a queue of its own and put all later ones
     * together on another - and kernels of two streams on one queue run one after the other.  Round 3's separate rate stream therefore shared the front stream's
     * queue (timeline of c5: 2.9 of the call's 3.0 ms on that one queue).  A rate chain that leaves the caller's stream now runs ON one of the two side streams,
     * chosen per call (enc_pipelined): the same packets in the same queue, by choice instead of by creation order. */
    for (int i = 0; i < c->opt.stream_skip; i++) { hipStream_t d; HIPCHK(hipStreamCreateWithFlags(&d, hipStreamNonBlocking)); }      /* diagnostic: shifts the assignment (never destroyed) */
    int plo = 0, phi = 0; (void)hipDeviceGetStreamPriorityRange(&plo, &phi);       /* least, greatest */
    const int prio = c->opt.side_prio == 1 ? plo : c->opt.side_prio == 2 ? phi : 0;
    if (c->opt.stream_order) { HIPCHK(hipStreamCreateWithPriority(&c->s_fr, hipStreamNonBlocking, prio)); HIPCHK(hipStreamCreateWithPriority(&c->s_pre, hipStreamNonBlocking, prio)); }
    else { HIPCHK(hipStreamCreateWithPriority(&c->s_pre, hipStreamNonBlocking, prio)); HIPCHK(hipStreamCreateWithPriority(&c->s_fr, hipStreamNonBlocking, prio)); }
    /* LC3PLUS_ENC_STREAMS=5: the pitch kernel and the one-frame-per-lane kernels on streams of their own (pays only where the HIP runtime has
     * hardware queues for them: GPU_MAX_HW_QUEUES >= 6) */
    c->s_pit = c->s_pre; c->s_ln = c->s_fr;
    if (c->opt.streams5) { HIPCHK(hipStreamCreateWithFlags(&c->s_pit, hipStreamNonBlocking)); HIPCHK(hipStreamCreateWithFlags(&c->s_ln, hipStreamNonBlocking)); }
    for (int i = 0; i < LC3D_MAX_RUNS; i++) { HIPCHK(hipEventCreateWithFlags(&c->ev_h[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_m[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_v[i], hipEventDisableTiming)); }
    for (int i = 0; i < 2; i++) { c->s_pk[i] = NULL; HIPCHK(hipEventCreateWithFlags(&c->ev_pk[i], hipEventDisableTiming)); }
    HIPCHK(hipEventCreateWithFlags(&c->ev_rate, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < LC3D_SETS; i++) HIPCHK(hipEventCreateWithFlags(&c->ev_done[i], hipEventDisableTiming));
    for (int i = 0; i < LC3D_MAX_RUNS; i++) { HIPCHK(hipEventCreateWithFlags(&c->ev_p[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_f[i], hipEventDisableTiming)); }
    return 0;
}
/* what enc_pipelined decides once per call for its runs */
struct enc_runs {
    float* dspec; float* dfrec; float* xn_w; const float* xprev; int xprev_stride; bool five;
    hipStream_t rts, rs; int hb, hk;      /* rts: the side stream of the rate chain (NULL: the caller's stream), rs: where the last rate kernel ran; the pre-kernels have run up to frame hb, in hk pieces */
};
/* run k of the pipelined path: frames tb ... tb + nt - 1 of the launch, Tr frames to a run */
static int enc_run(lc3hip_ctx* c, const enc_call* q, enc_runs* r, int k, int tb, int nt, int Tr)
{
    hipStream_t s = q->s;
    const int n_frames = q->n_frames, dT = q->dT, dt0 = q->dt0, mc = q->mc;
    float* dspec = r->dspec; float* dfrec = r->dfrec;
    /* The 12.8 kHz pre-kernels run ahead in larger pieces than the runs: the HP50 kernel (one stream per lane, B / 64 waves) costs ~0.1 ms
     * per launch whatever the frame count, which per run would make its stream the slowest.  First piece = the first run (the rate
     * kernel should start early), then three runs at a time, in stream order between the pitch kernels that need them.  (More side
     * streams than these two do not help: HIP multiplexes streams onto a few hardware queues and kernels of two streams that share
     * one run back to back.) */
    if (tb >= r->hb) {
        const int prn = c->opt.pre_runs;
        const int hn0 = r->hk == 0 ? Tr : prn * Tr, hn = n_frames - r->hb < hn0 ? n_frames - r->hb : hn0;
        DUPL('r') launch_resample(c, c->s_pre, q->dpcm, q->bitdepth, n_frames, r->hb, hn, mc, q->dy12, r->xprev, r->xprev_stride, q->cnt);
        DUPL('h') launch_hp50(c, c->s_pre, n_frames, r->hb, hn, mc, q->dy12, q->cnt);
        HIPCHK(hipGetLastError());
        r->hb += hn; r->hk++;
        if (r->five) { HIPCHK(hipEventRecord(c->ev_h[k], c->s_pre)); HIPCHK(hipStreamWaitEvent(c->s_pit, c->ev_h[k], 0)); }
    }
    /* OLPA + LTPF: two streams per wave where the 12.8 kHz frame length has such a kernel (LC3PLUS_ENC_PITCH2=0: one stream per wave) */
    /* (a ragged call: one stream per wave - the two streams of a pitch2 wave share barriers and have counts of their own) */
    const bool p2 = c->opt.pitch2 && (c->len12 == 128 || c->len12 == 64 || c->len12 == 32) && !q->cnt;
    auto pk = !p2 ? lc3_enc_pitch_kernel : c->len12 == 128 ? lc3_enc_pitch2_kernel : c->len12 == 64 ? lc3_enc_pitch2_kernel_l64 : lc3_enc_pitch2_kernel_l32;
    auto pitch = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3((unsigned)(p2 ? (c->ncs + 1) / 2 : c->ncs)), dim3(WAVE), 0, c->s_pit, c->d_plan, c->d_chans, c->d_state, c->state_words, mc, q->dy12, n_frames, tb, nt, c->ncs, dfrec, dT, dt0, ragged...); };
    if (q->cnt) pitch(lc3_enc_pitch_kernel_rag, q->cnt); else DUPL('p') pitch(pk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_p[k], c->s_pit));
    const int scf_wave = c->opt.scf_wave;
    {   /* the front: four frames a wave at 48 kHz / 10 ms, fm_frames a wave for the short frame lengths, else fpw frames a wave */
        const int fpw = nt < FRONT_FPW ? nt : FRONT_FPW;
        const int f4 = c->opt.front4;
        auto front4 = [&](auto kern, auto... placed) { LC3_LAUNCH(kern, dim3((unsigned)c->ncs * (unsigned)((nt + 3) / 4)), dim3(WAVE), 0, c->s_fr, c->d_plan, c->d_chans, c->d_state, q->dpcm, q->bitdepth, n_frames, tb, nt, c->ncs, dspec, c->srow, dT, dt0, dfrec, r->xn_w, r->xprev, r->xprev_stride, placed...); };
        auto frontm = [&](auto kern, auto... placed) { LC3_LAUNCH(kern, dim3((unsigned)c->ncs * (unsigned)((nt + c->fm_frames - 1) / c->fm_frames)), dim3(WAVE), 0, c->s_fr, c->d_plan, c->d_chans, c->d_state, q->dpcm, q->bitdepth, n_frames, tb, nt, c->fm_frames, c->ncs, dspec, c->srow, dT, dt0, dfrec, r->xn_w, r->xprev, r->xprev_stride, placed...); };
        auto front = [&](auto kern, auto... placed) { LC3_LAUNCH(kern, dim3((unsigned)c->ncs * (unsigned)((nt + fpw - 1) / fpw)), dim3(WAVE), 0, c->s_fr, c->d_plan, c->d_chans, c->d_state, q->dpcm, q->bitdepth, n_frames, tb, nt, fpw, c->ncs, dspec, c->srow, dT, dt0, dfrec, r->xn_w, r->xprev, r->xprev_stride, scf_wave, placed...); };
        if (f4 && !c->big && !scf_wave && c->N == 480 && c->la == 180 && (c->ylen & 15) == 0) {
            if (q->cnt) { if (q->placed) front4(lc3_enc_front4_kernel_plc_rag, c->plo, c->plcap, q->cnt); else front4(BY_FMT_RAG(q, lc3_enc_front4_kernel), q->cnt); }
            else if (q->placed) front4(lc3_enc_front4_kernel_plc, c->plo, c->plcap); else DUPL('f') front4(BY_FMT(q, lc3_enc_front4_kernel));
        } else if (f4 && c->fm_frames && !scf_wave) {
            if (q->cnt) { if (q->placed) frontm(lc3_enc_frontm_kernel_plc_rag, c->plo, c->plcap, q->cnt); else frontm(BY_FMT_RAG(q, lc3_enc_frontm_kernel), q->cnt); }
            else if (q->placed) frontm(lc3_enc_frontm_kernel_plc, c->plo, c->plcap); else frontm(BY_FMT(q, lc3_enc_frontm_kernel));
        }
        else if (q->cnt) { if (q->placed) front(lc3_enc_front_kernel_plc_rag, c->plo, c->plcap, q->cnt); else front(BY_FMT_RAG(q, lc3_enc_front_kernel), q->cnt); }      /* (standard layout: enc_launch) */
        else if (q->placed) front(c->big ? lc3_enc_front_kernel_big_plc : lc3_enc_front_kernel_plc, c->plo, c->plcap);
        else if (c->big) front(BY_FMT(q, lc3_enc_front_kernel_big));
        else DUPL('f') front(BY_FMT(q, lc3_enc_front_kernel));
    }
    HIPCHK(hipEventRecord(c->ev_m[k], c->s_fr));                 /* the MDCT memory hand-over and the spectrum rows of the run are written */
    if (r->five) HIPCHK(hipStreamWaitEvent(c->s_ln, c->ev_m[k], 0));
    const int fuse_vq = !scf_wave && !c->any_attack && c->opt.fuse_vq;
    const unsigned lanes = (unsigned)(((long long)c->ncs * nt + WAVE - 1) / WAVE);      /* waves of a kernel that takes one frame per lane */
    auto scf = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3(lanes), dim3(WAVE), 0, c->s_ln, c->d_plan, dT, dt0 + tb, nt, c->ncs, dspec, c->srow, dfrec, fuse_vq, ragged...); };
    auto attack = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3((unsigned)((c->ncs + WAVE - 1) / WAVE)), dim3(WAVE), 0, c->s_ln, c->d_plan, c->d_chans, c->d_state, c->state_words, LC3D_ST_SCAL(mc), dfrec, dT, dt0, tb, nt, c->ncs, ragged...); };
    auto snsvq = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3(lanes), dim3(WAVE), 0, c->s_ln, c->d_plan, dfrec, dT, dt0, tb, nt, c->ncs, c->any_attack, ragged...); };
    if (!scf_wave) { if (q->cnt) scf(lc3_enc_scf_lane_kernel_rag, q->cnt); else DUPL('e') scf(lc3_enc_scf_lane_kernel); }
    if (c->any_attack) { if (q->cnt) attack(lc3_enc_attack_kernel_rag, q->cnt); else attack(lc3_enc_attack_kernel); }
    if (!fuse_vq) { if (q->cnt) snsvq(lc3_enc_snsvq_kernel_rag, q->cnt); else DUPL('v') snsvq(lc3_enc_snsvq_kernel); }
    hipStream_t rs;
    {   /* shaping, TNS and the stateless half of the gain estimate: frame-parallel, behind the quantiser (LC3PLUS_ENC_SHAPE_ON_S=1, diagnostic: on the
         * launch stream in front of the rate kernel instead) */
        const int sfpw = c->opt.shape_fpw ? c->opt.shape_fpw : SHAPE_FPW, son = c->opt.shape_on_s;
        const int spw = nt < sfpw ? nt : sfpw;
        const unsigned sruns = (unsigned)((nt + spw - 1) / spw);
        /* LC3PLUS_ENC_SHAPE_ON_PITCH=1 (diagnostic): the shape kernel on the pitch stream, behind the pitch kernel, waiting for the quantiser's event.  Tried for c96, whose
         * front stream is the longest (3.6 of a 3.6 ms call) and whose pitch stream the lightest (1.4): the next call's pitch chain then queues behind a shape kernel that
         * waits for the front stream - 37.3 -> 31.0 Mframes/s; c1 111 -> 101, c5 97 -> 81, c3 93 -> 83; only c4 - long calls of 2.5 ms high-resolution frames, four runs per call, the front stream 8.5 of the 8.6 ms - gains (122.0 -> 126.1): on for that shape only. */
        const bool sop = !son && (c->opt.shape_on_pitch >= 0 ? c->opt.shape_on_pitch == 1 : (c->hr && c->N == 240 && n_frames >= 128));      /* c4's shape: calls of 128 / 256 frames 123.8 -> 126.0, 122.0 -> 126.1 */
        hipStream_t ss = son ? s : sop ? c->s_pit : c->s_ln;
        rs = (son || !r->rts) ? s : r->rts;
        if (son) { HIPCHK(hipEventRecord(c->ev_f[k], c->s_ln)); HIPCHK(hipStreamWaitEvent(s, c->ev_f[k], 0)); }
        if (sop) { HIPCHK(hipEventRecord(c->ev_v[k], c->s_ln)); HIPCHK(hipStreamWaitEvent(ss, c->ev_v[k], 0)); }
        const int swave = c->opt.shape_wave;
        if (q->dbw && bw_to(c, ss)) return 1;
        /* one frame per lane, or (LC3PLUS_ENC_SHAPE_WAVE=1) spw frames per wave; with per-frame bandwidths the _vbw twin of either */
        auto lane = [&](auto kern, auto... bw) { LC3_LAUNCH(kern, dim3(lanes), dim3(WAVE), 0, ss, c->d_plan, c->d_chans, dT, dt0 + tb, nt, c->ncs, dspec, c->srow, dfrec, bw...); };
        auto wave = [&](auto kern, auto... bw) { LC3_LAUNCH(kern, dim3((unsigned)c->ncs * sruns), dim3(WAVE), 0, ss, c->d_plan, c->d_chans, dT, dt0 + tb, nt, spw, c->ncs, dspec, c->srow, dfrec, bw...); };
        if (q->cnt) { if (q->dbw) lane(lc3_enc_shape_lane_kernel_vbw_rag, q->dbw, q->cnt); else lane(lc3_enc_shape_lane_kernel_rag, q->cnt); }      /* (never with LC3PLUS_ENC_SHAPE_WAVE: enc_launch) */
        else if (!swave) { if (q->dbw) lane(lc3_enc_shape_lane_kernel_vbw, q->dbw); else DUPL('a') lane(lc3_enc_shape_lane_kernel); }
        else if (q->dbw) wave(lc3_enc_shape_kernel_vbw, q->dbw);
        else if (c->big) wave(lc3_enc_shape_kernel_big);
        else DUPL('a') wave(lc3_enc_shape_kernel);
        HIPCHK(hipGetLastError());
        if (!son) { HIPCHK(hipEventRecord(c->ev_f[k], ss)); HIPCHK(hipStreamWaitEvent(rs, c->ev_f[k], 0)); }
    }
    HIPCHK(hipStreamWaitEvent(rs, c->ev_p[k], 0));
    if (k == 0 && c->rate_armed) HIPCHK(hipStreamWaitEvent(rs, c->ev_rate, 0));      /* the rate chain is a chain: behind the previous call's, whichever stream that ran on */
    const int last = tb + nt >= n_frames;            /* behind the last frame of this launch the MDCT memory goes into the state */
    auto rate = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3((unsigned)((c->ncs + RATE_WG - 1) / RATE_WG)), dim3(RATE_WG * WAVE), 0, rs, c->d_plan, c->d_chans, c->d_state, dT, dt0 + tb, nt, c->ncs, dspec, c->srow, dfrec, r->xn_w, last, ragged...); };
    if (q->cnt) rate(lc3_enc_rate_kernel_rag, q->cnt); else if (c->big) rate(lc3_enc_rate_kernel_big); else DUPL('s') rate(lc3_enc_rate_kernel);
    HIPCHK(hipGetLastError());
    r->rs = rs;
    return 0;
}
/* The pipelined path.  Per run of frames: on one side stream the pitch chain (resampler per frame, HP50 one stream per lane, OLPA +
 * LTPF one stream per wave); on another the frame-parallel front (MDCT ... scale factors), the attack decision and the SNS quantiser
 * (one frame per lane); on the launch stream the shape kernel (SNS shaping, TNS, log energies: frame-parallel) and behind it the rate
 * chain (lc3_enc_rate_kernel: rate loop, bisection, first quantisation), which also waits for the pitch chain.  Everything behind the
 * chain - gain adjustment, second quantisation, noise level, residual - is frame-parallel again and runs one frame per lane at the head
 * of the bitstream writer, once per call.  The side kernels of run k+1 are resident beside the launch stream's kernels of run k. */
static int enc_pipelined(lc3hip_ctx* c, enc_call* q)
{
    hipStream_t s = q->s;
    const int n_frames = q->n_frames, dT = q->dT, dt0 = q->dt0, hb_ = q->set;
    if (enc_side_streams(c)) return 1;
    enc_runs r;
    r.dspec = c->d_spec[hb_]; r.dfrec = c->d_frec[hb_];
    c->last_frec = r.dfrec; c->last_frec_frames = dT;
    const int runf = c->opt.run_frames ? c->opt.run_frames : c->input_ready ? LC3D_RUN_FRAMES_READY : LC3D_RUN_FRAMES;
    int R = (n_frames + runf - 1) / runf;              /* runs of frames */
    if (R > LC3D_MAX_RUNS) R = LC3D_MAX_RUNS;
    if (R < 1) R = 1;
    if (c->opt.runs) R = c->opt.runs;
    const int Tr = (n_frames + R - 1) / R;
    /* Where the side kernels of this call may start.  Normally behind everything the caller queued on s before the call (the PCM may
     * come from there).  With lc3hip_set_input_ready - the PCM of a call is complete when the call is made - and a previous call of
     * the same shape on the same stream, they need not wait for that call's chain and bitstream writer: their streams carry on in
     * their own order, writing the other set of rows and records (the set they write now was last read by the writer of the call before
     * the previous one: ev_done); the MDCT memory before frame 0 is read from the previous call's hand-over (two alternating buffers),
     * not from the state that call's last rate kernel is still to update. */
    const int amax = c->opt.ahead_max ? c->opt.ahead_max : LC3D_AHEAD_MAX_FRAMES;
    /* A configuration copy queued behind the previous call (lc3hip_upload_chans_async) is on s, which a call that overlaps does not wait for: only a
     * per-frame-bandwidth call overlaps it, and only when that copy changed nothing but the bandwidth words, which its kernels do not read (the other words
     * are rewritten with their own values).  A call that forks from s is behind the copy, and so is everything after it. */
    const bool cfg_ok = c->cfg_fresh == 0 || (c->cfg_fresh == 1 && q->dbw);
    const bool ahead = c->input_ready && n_frames <= amax && c->ahead_ok && c->ahead_T == n_frames && c->ahead_R == R && c->last_stream == s && dt0 == 0 && dT == n_frames && q->pack && cfg_ok && !q->cnt;
    if (!ahead) c->cfg_fresh = 0;
    r.xn_w = c->d_xnext[c->xn_par];                         /* written by this call's front kernel */
    /* one buffer more than calls in flight: the one written now was last read by the call LC3D_SETS back (its resampler and front) and by the
     * rate kernel of the call before that, all finished before the bitstream writer this call's side streams have waited for */
    r.xprev = ahead ? c->d_xnext[(c->xn_par + LC3D_SETS) % (LC3D_SETS + 1)] : c->d_state + LC3D_ST_XPREV;
    r.xprev_stride = ahead ? q->mc : c->state_words;
    const bool five = r.five = c->s_pit != c->s_pre;
    /* The rate chain on a stream of its own, so that the rate kernel of call k+1 runs beside the bitstream writer of call k (which stays on the
     * caller's stream: it is what the caller waits for).  It pays where the caller's stream - rate kernel + writer - is the longest of the three:
     * large frames (the writer's work grows with the bytes: c96 22 -> 32 Mframes/s, c5 77 -> 83) and short calls (c3 +3 %); on 80-byte frames in
     * calls of 64 (c1) a fourth side stream costs 0 ... 11 % (it shares one of HIP's four hardware queues with another, depending on what else the
     * process created), and on c4 4 %.  LC3PLUS_ENC_RATE_STREAM=0 / 1 forces the choice (diagnostic). */
    const int rt_env = c->opt.rate_stream;
    const bool want_rt = rt_env == 1 || (rt_env < 0 && !c->big && (c->mean_nbytes >= 120 || n_frames <= 32));      /* large layout (c96, with round 4's writer): 36.6 on the caller's stream against 33.9 / 34.5 on the front / pitch stream */
    /* ... and then on which side stream: behind the pitch kernel (it waits for the shape kernel's event) or behind the shape kernel (it waits for the pitch kernel's).
     * Measured (Mframes/s, front stream / pitch stream): 48 kHz / 10 ms x 64 frames at 120 bytes 91.6 / 102.5, 160: 88.5 / 98.0, 240: 82.0 / 88.0, 400: 72.8 / 75.2, c5 88.3 / 97.1 (calls of
     * 32: 82.7 / 88.5); 80-byte frames in calls of 6: 51.3 / 60.4, 8: 62.3 / 68.1, 12: 72.4 / 88.6, 14: 80.6 / 88.4, 18: 85.3 / 90.8, 28: 93.4 / 95.5, 32: 94.6 / 100.9 - but of 16: 94.2 / 92.6 (c3 94.1 / 89.8),
     * 20: 93.8 / 91.0, 24: 96.4 / 92.9, and c96 32.8 / 30.8.  The pitch stream is the lighter one; behind the shape kernel the rate kernel blocks nothing while it waits, which wins where the
     * front stream is at its best (calls of 16 ... 24 frames in whole groups of four - lc3_enc_front4_kernel's unit) and in the large layout. */
    const bool on_pre = c->opt.rate_on >= 0 ? c->opt.rate_on == 1 : !(c->big || (c->mean_nbytes < 120 && n_frames >= 16 && n_frames <= 24 && (n_frames & 3) == 0));
    r.rts = want_rt ? (on_pre ? c->s_pit : c->s_ln) : NULL;          /* NULL: the rate kernels run on the caller's stream */
    if (!ahead) {
        HIPCHK(hipEventRecord(c->ev_fork, s)); HIPCHK(hipStreamWaitEvent(c->s_pre, c->ev_fork, 0)); HIPCHK(hipStreamWaitEvent(c->s_fr, c->ev_fork, 0));
        if (five) { HIPCHK(hipStreamWaitEvent(c->s_pit, c->ev_fork, 0)); HIPCHK(hipStreamWaitEvent(c->s_ln, c->ev_fork, 0)); }
    } else {
        /* The previous call's last run: the index it made last (ahead_last), not R - 1.  A call makes ceil(n / Tr) runs, which equals R for every n with the default
         * run lengths (tests/test_call_shapes_cpu.py: the run invariant) - the two indices are then the same - but not with LC3PLUS_ENC_RUN_FRAMES or LC3PLUS_ENC_RUNS
         * (run length 1, n = 20: R = 16, Tr = 2, ten runs), where ev_m[R - 1] is an event of some earlier call or of none. */
        HIPCHK(hipStreamWaitEvent(c->s_pre, c->ev_m[c->ahead_last], 0));    /* the resampler reads the hand-over the previous call's last front kernel wrote */
        HIPCHK(hipStreamWaitEvent(c->s_pre, c->ev_done[hb_], 0)); HIPCHK(hipStreamWaitEvent(c->s_fr, c->ev_done[hb_], 0));
        if (five) { HIPCHK(hipStreamWaitEvent(c->s_pit, c->ev_done[hb_], 0)); HIPCHK(hipStreamWaitEvent(c->s_ln, c->ev_done[hb_], 0));
                    if (c->any_attack) HIPCHK(hipStreamWaitEvent(c->s_fr, c->ev_f[c->ahead_last], 0)); }      /* the front reads the attack detector's filter memory the previous call's attack kernel leaves */
    }
    r.rs = s; r.hb = 0; r.hk = 0;                         /* rs: where the rate kernels run */
    int made = 0;                                         /* runs made: ceil(n_frames / Tr), at most R */
    for (int tb = 0; tb < n_frames; made++, tb += Tr)
        if (enc_run(c, q, &r, made, tb, n_frames - tb < Tr ? n_frames - tb : Tr, Tr)) return 1;
    HIPCHK(hipEventRecord(c->ev_rate, r.rs)); c->rate_armed = 1; q->rate_on_side = r.rs != s;
    if (r.rs != s) HIPCHK(hipStreamWaitEvent(s, c->ev_rate, 0));      /* the writer (and whatever the caller queues next) behind the rate chain */
    /* a ragged call forks from s and lets nothing overlap it: it fills the hand-over only for the streams that had a frame, so the call behind it reads the MDCT memory from the state */
    c->ahead_ok = (dt0 == 0 && dT == n_frames && q->pack && !q->cnt) ? 1 : 0; c->ahead_T = n_frames; c->ahead_R = R; c->ahead_last = made - 1;
    c->xn_par = (c->xn_par + 1) % (LC3D_SETS + 1);
    return 0;
}
/* the bitstream writer over all dT frames of the call, once the last launch of the call has filled the hand-over; on the pipelined path it starts from the shaped
 * spectra (frame-parallel tail, one frame per lane) */
static int enc_writer(lc3hip_ctx* c, const enc_call* q)
{
    hipStream_t s = q->s;
    const int dT = q->dT; const bool split = q->split;
    float* rows_for_pack = split ? c->d_spec[q->set] : nullptr; const float* frec_for_pack = split ? c->d_frec[q->set] : nullptr;
    HIPCHK(hipGetLastError());
    const int wpg = c->opt.pack_wpg;                  /* waves per workgroup of the writer (they share the coder's tables in LDS) */
    const size_t per_wave = (size_t)PK_XBUF * WAVE * sizeof(unsigned);
    const long long tasks = (long long)c->ncs * dT, per_wg = (long long)wpg * WAVE;
    /* The writer codes one frame per lane: its duration is the latency of the LARGEST frame of the batch (c5: 1.7 ms for 400 bytes, c96: 3.2 ms), whatever the
     * batch size, and on the caller's stream the writers of consecutive calls run one after the other.  Where that is the longest stream (the rule that moves the
     * rate chain off the caller's stream: large frames, short calls) and calls overlap, the writers CAN alternate between two side streams - writer k + 1 beside
     * writer k, each with its own set of scratch rows and status bytes, the caller's stream waiting for their events in call order.  Measured (Mframes/s,
     * off / on): with HIP's default four hardware queues c5 87.0 / 80.0, c96 32.1 / 28.7, c3 85.1 / 73.0 - six streams share four queues and kernels of two
     * streams on one queue run back to back; with GPU_MAX_HW_QUEUES=8 c5 90.9 / 92.4, c96 28.8 / 33.9, c3 85.5 / 85.8.  So it is a deployment switch
     * (LC3PLUS_ENC_PACK_STREAM=1 together with GPU_MAX_HW_QUEUES >= 6), off by default. */
    const int pk_env = c->opt.pack_stream;
    const bool side = split && q->rate_on_side && c->input_ready && q->dt0 == 0 && dT == q->n_frames && pk_env == 1;
    hipStream_t ps = s;
    if (side) {
        /* behind this call's rate chain only - NOT behind the caller's stream, whose tail is the writer of the call before: under the input-ready promise the
         * output buffer of a call, like its PCM, is the caller's to have ready (include/lc3plus_batch.h) */
        if (!c->s_pk[c->pk_par]) HIPCHK(hipStreamCreateWithFlags(&c->s_pk[c->pk_par], hipStreamNonBlocking));
        ps = c->s_pk[c->pk_par];
        HIPCHK(hipStreamWaitEvent(ps, c->ev_rate, 0));
    }
    if (side && c->pk.on) HIPCHK(hipStreamWaitEvent(ps, c->ev_scan, 0));     /* packed output: behind the call's scan (the table the writers read) */
    if (split) HIPCHK(hipMemsetAsync(c->d_status, 0, (size_t)c->ncs * dT, ps));
    /* large frames: tail + writer a frame per wave (lc3_enc_tailw_kernel, lc3_enc_rate.inc), launched first - its waves are the long ones */
    const int big_from = (split && c->opt.tailw_bytes && c->max_nbytes >= c->opt.tailw_bytes && !c->pk.on) ? c->opt.tailw_bytes : 0;   /* (no packed form) */
    if (big_from) {
        const int fpw = dT < 4 ? dT : 4;
        const unsigned wruns = (unsigned)((dT + fpw - 1) / fpw);
        LC3_LAUNCH(c->big ? lc3_enc_tailw_kernel_big : lc3_enc_tailw_kernel, dim3((unsigned)c->ncs * wruns), dim3(WAVE), 0, ps, c->d_plan, c->d_chans, dT, dT, fpw, c->ncs, rows_for_pack, c->srow, frec_for_pack, q->dout,
                           q->out_stride, c->d_status, big_from);
        HIPCHK(hipGetLastError());
    }
    const bool two = split && c->opt.pack_split == 1;
    if (!big_from || c->min_nbytes < big_from) {
        const dim3 grid((unsigned)((tasks + per_wg - 1) / per_wg)), block(wpg * WAVE);
        const size_t dyn = per_wave * wpg + ((size_t)(c->opt.pack_pad_kb > 0 ? c->opt.pack_pad_kb : 0) << 10);
        const long long* pt = c->pk.on || q->cnt ? c->pk.tab : nullptr;      /* packed output: the _pk twins write each frame at its offset of the call's table (a ragged call always has one: the scan's, or the plan kernel's slots) */
        auto writer = [&](auto kern, size_t lds, auto... poff) { LC3_LAUNCH(kern, grid, block, lds, ps, c->d_plan, c->d_chans, q->ddump, q->dstride, dT, 0, dT, c->ncs, q->dout, pt ? 0 : q->out_stride, c->d_status, rows_for_pack, c->srow, frec_for_pack, big_from, poff...); };
        if (two) {       /* LC3PLUS_ENC_PACK_SPLIT=1: the writer as two kernels (head, coder) */
            if (pt) { writer(lc3_enc_pack_head_kernel_pk, 0, pt); writer(lc3_enc_pack_code_kernel_pk, dyn, pt); }
            else { writer(lc3_enc_pack_head_kernel, 0); writer(lc3_enc_pack_code_kernel, dyn); }
        } else {
            /* 96 or 128 registers (lc3_enc_pack.inc, the table at lc3_enc_pack_kernel_w5): five waves per SIMD pay for long calls of small 10 ms frames */
            const bool w5 = c->opt.pack_w5 >= 0 ? c->opt.pack_w5 == 1 : (split && !c->big && !c->hr && c->N == 480 && dT >= 48 && c->max_nbytes <= 100);
            if (q->cnt) { if (w5) writer(lc3_enc_pack_kernel_w5_pk_rag, dyn, pt, q->cnt); else writer(lc3_enc_pack_kernel_pk_rag, dyn, pt, q->cnt); }
            else if (pt) writer(w5 ? lc3_enc_pack_kernel_w5_pk : lc3_enc_pack_kernel_pk, dyn, pt);
            else DUPL('k') writer(w5 ? lc3_enc_pack_kernel_w5 : lc3_enc_pack_kernel, dyn);
        }
    }
    if (split && c->input_ready) { HIPCHK(hipEventRecord(c->ev_done[c->row_par], ps)); c->row_par = (c->row_par + 1) % LC3D_SETS; }      /* this call's set of rows and records is free again */
    if (side) { HIPCHK(hipEventRecord(c->ev_pk[c->pk_par], ps)); HIPCHK(hipStreamWaitEvent(s, c->ev_pk[c->pk_par], 0)); c->pk_par ^= 1; }
    return 0;
}
static int enc_launch(lc3hip_ctx* c, const void* dpcm, int bitdepth, int n_frames, uint8_t* dout, int out_stride, hipStream_t s, lc3d_trace* dtr,
                      int dT, int dt0, bool pack, const uint16_t* dfsz, const uint16_t* dbw)
{
    /* two kernels: lc3_encode_kernel (one wave per channel-stream, frames in order) leaves each frame's parameters and quantised
     * spectrum in a record; lc3_enc_pack_kernel (one channel-frame per lane, any frame size) writes the bytes.  With stage traces,
     * or with LC3PLUS_ENC_FUSED=1 (diagnostic), the first kernel writes the bytes itself. */
    /* A call of very few frames is latency bound and the one-frame-per-lane writer is the longest chain in it (~0.19 ms for a frame of
     * 80 bytes whatever the batch size): up to LC3D_FUSED_MAX_T frames per call the wave-parallel writer inside the first kernel
     * (st_bitstream, ~6 us per frame) is used instead - the single-stream lc3_enc_* API and T = 1 batches live here. */
    enc_call q = {dpcm, bitdepth, n_frames, dout, out_stride, s, dtr, dT, dt0, pack, dfsz, dbw};
    q.set = c->input_ready ? c->row_par : 0;        /* the set of hand-over buffers of this call (rows, records, writer scratch, status bytes) */
    /* with the input-ready promise consecutive short calls overlap on the pipelined path, which then wins from 4 frames per call
     * (4096 streams, Mframes/s pipelined / in-kernel writer: 3 frames 31.9 / 36.3, 4: 39.8 / 38.0, 6: 48.6 / 40.2, 8: 53.9 / 41.2; without the
     * promise 8: 40.2 / 41.2) */
    /* (per-frame bitrates: always - lc3_encode_kernel_var reloads the configuration per frame; it is the only kernel that does) */
    /* the PCM formats beyond the reference's three have kernels of their own (_fmt) wherever the load could not be added without moving the registers of the kernel that is there */
    q.fmt_plain = bitdepth == 16 || bitdepth == 24 || bitdepth == 32;
    q.fmt_wire = lc3d_pcm_type_wire(bitdepth & LC3D_PCM_TYPE_MASK) != 0;           /* the wire sample types: the _wire twins, so that the _fmt kernels stay what they were */
    q.placed = c->plo != nullptr;                                                  /* placed PCM: the _plc twins, one form for every sample type */
    q.cnt = c->rag ? c->d_cnt : nullptr;                                           /* ragged (lc3hip_encode_rates_device): its plan kernel always writes sizes and a table of offsets */
    if (q.cnt && (!dfsz || dtr || dt0 != 0 || dT != n_frames)) return 1;
    /* A ragged call takes the pipelined path where the dense call without the input-ready promise does: no per-frame bitrates (with them the dense call runs the
     * one-wave kernel too; without them the sizes are the configuration's, which is what the pipeline's kernels read), standard layout, more than LC3D_FUSED_MAX_T
     * frames - with or without the promise, whose lower threshold exists because calls overlap there, and a ragged call does not - and none of the diagnostic kernel
     * variants, which have no ragged forms.  Every other ragged call: the one-wave _rag kernels.  LC3PLUS_ENC_RAGGED_PIPE=0: all of them. */
    q.rag_pipe = q.cnt && c->rag == 2 && c->opt.ragged_pipe && !c->big && n_frames > LC3D_FUSED_MAX_T && !c->fused && !c->opt.no_split && !c->opt.shape_wave &&
                 c->opt.pack_split != 1 && !c->opt.tailw_bytes && !c->opt.scf_wave;
    if (q.rag_pipe) q.dfsz = dfsz = nullptr;
    if (q.placed && (dt0 != 0 || dT != n_frames || (bitdepth & LC3D_PCM_CHANNEL_MAJOR))) return 1;    /* the offsets are indexed by the call's frames; the host refuses the rest */
    const bool in_kernel_writer = dtr || c->fused || dfsz || dT <= (c->input_ready ? LC3D_FUSED_MAX_T_READY : LC3D_FUSED_MAX_T);
    q.mc = c->big ? LC3D_MEMCAP_BIG : LC3D_MEMCAP_STD;
    if (enc_size_set(c, &q, in_kernel_writer)) return 1;
    if (q.split ? enc_pipelined(c, &q) : enc_one_wave(c, &q)) return 1;
    if (q.ddump && pack && enc_writer(c, &q)) return 1;
    HIPCHK(hipGetLastError());
    c->last_stream = s;
    return 0;
}

static bool host_ptr_is_pinned(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

/* Host pointers on both sides (SURVEY 8d "wall-clock over the encode() call including H2D of PCM and D2H of bitstreams"): the PCM of a
 * call is cut into runs of frames (all streams advance together, so every run fills the GPU like the whole call would; cutting by
 * streams would not).  Run k+1 goes up on a copy stream while run k is encoded on the launch stream: PCM of a run is a strided block of
 * the caller's [stream][frame][channel][N] array - a 2-D copy (SDMA) straight from the caller's memory when that is pinned
 * (hipHostMalloc / hipHostRegister), otherwise rows are staged through the library's own pinned slots by the calling thread, which
 * overlaps with the GPU work of the previous run.  The bitstream writer runs ONCE behind the last run over all frames of the call (one
 * frame per lane makes it latency bound: per run it would cost as much as for the whole call), then the frames come down in one
 * linear copy.  State stays on the device between runs.  The first run is short so that the kernels start early. */
static int encode_host(lc3hip_ctx* c, const void* pcm, int bitdepth, int n_frames, void* out, int out_stride, hipStream_t s, const uint16_t* dfsz,
                       const uint16_t* dbw)
{
    const size_t bps = (size_t)lc3d_pcm_elem_bytes(bitdepth);
    const size_t fr_in = (size_t)c->channels * c->N * bps;                    /* bytes of one stream-frame of PCM */
    const size_t pcm_bytes = (size_t)c->n_streams * n_frames * fr_in, out_bytes = (size_t)c->n_streams * n_frames * out_stride;
    int K = (int)(pcm_bytes >> 25);                                           /* ~32 MB of PCM per run */
    if (K < 1) K = 1; if (K > 8) K = 8; if (K > n_frames) K = n_frames;
    if ((bitdepth & LC3D_PCM_CHANNEL_MAJOR) && c->channels > 1) K = 1;        /* a run of frames is one block per stream in the two other layouts only: this one goes up in one piece */
    if (!dfsz && (c->fused || n_frames <= LC3D_FUSED_MAX_T)) K = 1;                                          /* diagnostic single-kernel path: the first kernel addresses the output by its own frame count (the per-frame-bitrate kernel by the call's) */
    const int Tc = (n_frames + K - 1) / K, T0 = K > 1 ? (Tc + 1) / 2 : Tc;   /* first run: half a run */
    const bool pin_in = host_ptr_is_pinned(pcm);
    const size_t cin = (size_t)c->n_streams * Tc * fr_in;
    if (!c->s_h2d) {
        HIPCHK(hipStreamCreateWithFlags(&c->s_h2d, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) { HIPCHK(hipEventCreateWithFlags(&c->ev_h2d[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_k[i], hipEventDisableTiming)); }
    }
    /* the two chunk slots and the output: no wait for the device - a call through host pointers returns when its work is done */
    const lc3hip_buf dev[] = {{&c->hp_dpcm[0], cin, false}, {&c->hp_dpcm[1], cin, false}}, pin[] = {{&c->hp_pin_in[0], cin, true}, {&c->hp_pin_in[1], cin, true}};
    if (grow_group(&c->hp_pcm_cap, cin, dev, 2, false, &c->wk) || (!pin_in && grow_group(&c->hp_pin_in_cap, cin, pin, 2, false)) || grow(&c->d_out, &c->out_cap, out_bytes, out_bytes, false, &c->wk)) return 1;
    const size_t in_pitch = (size_t)n_frames * fr_in;
    HIPCHK(hipEventRecord(c->ev0, s));
    HIPCHK(hipMemsetAsync(c->d_out, 0, out_bytes, s));
    for (int k = 0, t0 = 0; t0 < n_frames; k++) {
        const int i = k & 1, want = k == 0 ? T0 : Tc, tc = n_frames - t0 < want ? n_frames - t0 : want;
        const size_t w_in = (size_t)tc * fr_in;
        if (k >= 2) HIPCHK(hipEventSynchronize(c->ev_k[i]));                   /* run k - 2 has been encoded: its staging slot is free */
        const uint8_t* src = (const uint8_t*)pcm + (size_t)t0 * fr_in;
        if (pin_in) HIPCHK(hipMemcpy2DAsync(c->hp_dpcm[i], w_in, src, in_pitch, w_in, (size_t)c->n_streams, hipMemcpyHostToDevice, c->s_h2d));
        else {
            for (int st = 0; st < c->n_streams; st++) memcpy((uint8_t*)c->hp_pin_in[i] + st * w_in, src + st * in_pitch, w_in);
            HIPCHK(hipMemcpyAsync(c->hp_dpcm[i], c->hp_pin_in[i], w_in * c->n_streams, hipMemcpyHostToDevice, c->s_h2d));
        }
        HIPCHK(hipEventRecord(c->ev_h2d[i], c->s_h2d));
        HIPCHK(hipStreamWaitEvent(s, c->ev_h2d[i], 0));
        if (enc_launch(c, c->hp_dpcm[i], bitdepth, tc, c->d_out, out_stride, s, nullptr, n_frames, t0, t0 + tc >= n_frames, dfsz, dbw)) return 1;
        HIPCHK(hipEventRecord(c->ev_k[i], s));
        t0 += tc;
    }
    HIPCHK(hipEventRecord(c->ev1, s));
    HIPCHK(hipMemcpyAsync(out, c->d_out, out_bytes, hipMemcpyDeviceToHost, s));
    SYNC_TIMED(c, s);
    return 0;
}

extern "C" int lc3hip_upload_enc_table(void* ctx, const lc3d_chan* tab, int n)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (replace(&c->d_etab, sizeof(lc3d_chan) * (size_t)n)) return 1;      /* no wait of its own: lc3_host.c uploads the table once, before the first call that reads it */
    HIPCHK(hipMemcpy(c->d_etab, tab, sizeof(lc3d_chan) * (size_t)n, hipMemcpyHostToDevice));
    c->etab_attack = 0; c->etab_max = n - 1;
    for (int i = 1; i < n; i++) c->etab_attack |= tab[i].attack_handling != 0;
    return 0;
}
/* the stream-frame sizes of a per-frame-bitrate call through pinned staging (stage_words) to the device, queued on s ahead of its kernels */
static int upload_fsz(lc3hip_ctx* c, const uint16_t* fsz_host, int n_frames, hipStream_t s, const uint16_t** dfsz, hipEvent_t* ev)
{
    const size_t fb = sizeof(uint16_t) * (size_t)c->n_streams * n_frames;
    int k;
    if (stage_words(&c->fsz, fsz_host, fb, &k, &c->wk)) return 1;
    HIPCHK(hipMemcpyAsync(c->fsz.d[k], c->fsz.h[k], fb, hipMemcpyHostToDevice, s));
    *dfsz = c->fsz.d[k]; *ev = c->fsz.ev[k];
    return 0;
}
/* the bandwidths in force of a per-frame-bandwidth call into pinned staging (stage_words); bw_to queues the copy */
static int stage_bw(lc3hip_ctx* c, const uint16_t* bw_host, int n_frames, const uint16_t** dbw, hipEvent_t* ev)
{
    const size_t fb = sizeof(uint16_t) * (size_t)c->n_streams * n_frames;
    int k;
    if (stage_words(&c->bw, bw_host, fb, &k, &c->wk)) return 1;
    if (!c->ev_bwcp) HIPCHK(hipEventCreateWithFlags(&c->ev_bwcp, hipEventDisableTiming));
    c->bw_src = c->bw.h[k]; c->bw_bytes = fb; c->bw_on = nullptr; c->pl.pending = 0;
    *dbw = c->bw.d[k]; *ev = c->bw.ev[k];
    return 0;
}
static int plan_launch(lc3hip_ctx* c, hipStream_t st);
/* packed output: the scan of the call's frame sizes on st (lc3_pack_sums_kernel, lc3_pack_base_kernel, lc3_pack_offsets_kernel) into tab, the caller's
 * offsets, total, flags (plan_flags: the plan kernel has written bits 0 ... 2 there) and num_bytes (where no plan kernel wrote them: plan_nb = 0) */
static int pack_scan(lc3hip_ctx* c, hipStream_t st, int T, int slot /* the plan set, LC3D_SETS without a plan kernel */, const uint16_t* fsz, const int4* pend,
                     int plan_flags, int plan_nb)
{
    const long long n = (long long)c->n_streams * T, nb = (n + PKS_TILE - 1) / PKS_TILE;
    long long* tab = c->d_poff[slot]; long long* bsum = c->d_pbsum + (size_t)slot * PKS_SUMS(c->poff_cap);
    PkSrc q; q.fsz = fsz; q.pend = fsz ? nullptr : pend; q.chans = c->d_chans; q.channels = c->channels; q.order = c->pk.order; q.S = c->n_streams; q.T = T;
    LC3_LAUNCH(lc3_pack_sums_kernel, dim3((unsigned)nb), dim3(PKS_THREADS), 0, st, q, n, bsum);
    LC3_LAUNCH(lc3_pack_base_kernel, dim3(1), dim3(PKS_THREADS), 0, st, bsum, nb, c->pk.total);
    LC3_LAUNCH(lc3_pack_offsets_kernel, dim3((unsigned)nb), dim3(PKS_THREADS), 0, st, q, n, (const long long*)bsum, c->pk.cap, tab, c->pk.offs,
                       c->pk.fl, plan_flags, plan_nb ? (int32_t*)nullptr : c->pk.nb);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_scan, st));
    c->pk.tab = tab;
    return 0;
}
static int bw_to(lc3hip_ctx* c, hipStream_t st)
{
    const int k = (c->bw.k + LC3D_SETS - 1) % LC3D_SETS;                      /* the slot stage_bw filled for this call */
    if (!c->bw_on) {
        if (c->pl.pending) { if (plan_launch(c, st)) return 1; }             /* words from device memory: the call's plan kernel writes them */
        else HIPCHK(hipMemcpyAsync(c->bw.d[k], c->bw_src, c->bw_bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(c->ev_bwcp, st)); c->bw_on = st;
    } else if (c->bw_on != st) HIPCHK(hipStreamWaitEvent(st, c->ev_bwcp, 0));
    return 0;
}
extern "C" int lc3hip_encode(void* ctx, const void* pcm, int pcm_on_device, int bitdepth, int n_frames, void* out, int out_stride,
                             int out_on_device, void* hip_stream, int sync, void* trace_host, const uint16_t* fsz_host, const uint16_t* bw_host)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (!hip_stream && !c->stream) HIPCHK(hipStreamCreate(&c->stream));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const uint16_t* dfsz = nullptr; hipEvent_t ev_fsz = nullptr;
    const uint16_t* dbw = nullptr; hipEvent_t ev_bw = nullptr;
    if (c->counts) return 1;                   /* per-stream frame counts: the calls with flags in device memory alone (the host refuses the others) */
    if (fsz_host && !c->d_etab) return 1;
    if (bw_host && c->big) return 1;            /* no large-layout kernels: that layout only serves high-resolution batches, which the host refuses */
    if (c->plo && (!pcm_on_device || trace_host)) return 1;      /* placed PCM: device-pointer calls without traces (the host refuses the others) */
    if (c->wk.calls && work_poison_all(&c->wk)) return 1;        /* once per call: a host-pointer call's pieces come behind it */
    if (!pcm_on_device && !out_on_device && !trace_host) {
        if (c->chans_armed) HIPCHK(hipStreamWaitEvent(s, c->ev_chans, 0));
        if (fsz_host && upload_fsz(c, fsz_host, n_frames, s, &dfsz, &ev_fsz)) return 1;
        if (bw_host && stage_bw(c, bw_host, n_frames, &dbw, &ev_bw)) return 1;
        if (encode_host(c, pcm, bitdepth, n_frames, out, out_stride, s, dfsz, dbw)) return 1;
        if (ev_fsz) HIPCHK(hipEventRecord(ev_fsz, s));
        if (ev_bw) HIPCHK(hipEventRecord(ev_bw, s));
        return 0;
    }
    const size_t bps = (size_t)lc3d_pcm_elem_bytes(bitdepth);
    const size_t pcm_bytes = (size_t)c->n_streams * n_frames * c->channels * c->N * bps;
    const size_t out_bytes = (size_t)c->n_streams * n_frames * out_stride;
    const void* dpcm = pcm; uint8_t* dout = (uint8_t*)out;
    if (!pcm_on_device) {
        if (grow(&c->d_pcm, &c->pcm_cap, pcm_bytes, pcm_bytes, false, &c->wk)) return 1;      /* staging of host arrays (d_pcm, d_out, d_trace): no wait of its own, as in encode_host */
        HIPCHK(hipMemcpyAsync(c->d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice, s));
        dpcm = c->d_pcm;
    }
    if (!out_on_device) {
        if (grow(&c->d_out, &c->out_cap, out_bytes, out_bytes, false, &c->wk)) return 1;
        dout = c->d_out;
        HIPCHK(hipMemsetAsync(dout, 0, out_bytes, s));
    }
    lc3d_trace* dtr = nullptr;
    if (trace_host) {
        const size_t tb = sizeof(lc3d_trace) * (size_t)c->ncs * n_frames;
        if (grow(&c->d_trace, &c->trace_cap, tb, tb, false, &c->wk)) return 1;
        HIPCHK(hipMemsetAsync(c->d_trace, 0, tb, s));
        dtr = c->d_trace;
    }
    if (c->opt.check_ready && c->input_ready && pcm_on_device) {
        /* The promise says the PCM is complete NOW.  What can be checked: if everything this library queued on s has finished and s still has work pending, that work is
         * the caller's - possibly the producer of this PCM.  (While our own work is pending nothing can be told apart; the check is a debug aid, not a proof.) */
        if (!c->ev_ours) { HIPCHK(hipEventCreateWithFlags(&c->ev_ours, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_now, hipEventDisableTiming)); }
        if ((!c->ours_armed || c->last_stream != s || hipEventQuery(c->ev_ours) == hipSuccess) && hipStreamQuery(s) == hipErrorNotReady) {
            fprintf(stderr, "lc3plus_hip: LC3PLUS_CHECK_READY: lc3plus_enc_batch_set_input_ready(1) is in force, but work queued by the caller is still pending on the stream "
                            "of this call - the PCM (or the output buffer) may not be ready; call refused\n");
            (void)hipGetLastError();
            return 1;
        }
        (void)hipGetLastError();
    }
    /* behind the LC3PLUS_CHECK_READY test, which must see no copy of ours pending on s */
    if (c->chans_armed) HIPCHK(hipStreamWaitEvent(s, c->ev_chans, 0));
    if (fsz_host && upload_fsz(c, fsz_host, n_frames, s, &dfsz, &ev_fsz)) return 1;
    if (bw_host && stage_bw(c, bw_host, n_frames, &dbw, &ev_bw)) return 1;
    HIPCHK(hipEventRecord(c->ev0, s));
    if (c->pk.on && (fsz_host || bw_host || pack_scan(c, s, n_frames, LC3D_SETS, nullptr, nullptr, 0, 0))) return 1;      /* packed output, no per-frame words */
    if (enc_launch(c, dpcm, bitdepth, n_frames, dout, out_stride, s, dtr, n_frames, 0, true, dfsz, dbw)) return 1;
    if (c->pk.on && placed_mark(c->plo, c->plcap, c->channels, c->N, (long long)c->n_streams * n_frames, c->pk.fl, LC3D_ENC_FL_PCM_PLACE, s)) return 1;
    HIPCHK(hipEventRecord(c->ev1, s));
    if (ev_fsz) HIPCHK(hipEventRecord(ev_fsz, s));
    if (ev_bw) HIPCHK(hipEventRecord(ev_bw, s));      /* the end of the call on s lies behind every kernel that read the words, on whichever stream */
    if (c->opt.check_ready && c->ev_ours) { HIPCHK(hipEventRecord(c->ev_ours, s)); c->ours_armed = 1; }
    if (!out_on_device) HIPCHK(hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, s));
    if (trace_host) HIPCHK(hipMemcpyAsync(trace_host, dtr, sizeof(lc3d_trace) * (size_t)c->ncs * n_frames, hipMemcpyDeviceToHost, s));
    if (sync || !out_on_device || trace_host) SYNC_TIMED(c, s);
    return 0;
}

/* the offset tables (one per plan set and one more) and, in one buffer, a slot of tile sums for each, for n frames */
static int pk_tables(lc3hip_ctx* c, size_t n)
{
    lc3hip_buf b[LC3D_SETS + 2];
    for (int i = 0; i < LC3D_SETS + 1; i++) b[i] = {(void**)&c->d_poff[i], n * sizeof(long long), false};
    b[LC3D_SETS + 1] = {(void**)&c->d_pbsum, (size_t)(LC3D_SETS + 1) * PKS_SUMS(n) * sizeof(long long), false};
    return grow_group(&c->poff_cap, n, b, LC3D_SETS + 2, true, &c->wk);
}
/* the pending call's plan kernel on st: behind the previous call's plan kernel (the carry), behind the call that used this set last, and - when it starts
 * from the configuration the host wrote - behind that write */
static int plan_launch(lc3hip_ctx* c, hipStream_t st)
{
    const int k = c->pl.k, T = c->pl.T;
    if (c->plan_armed) HIPCHK(hipStreamWaitEvent(st, c->ev_plan, 0));
    if (c->pset_armed[k]) HIPCHK(hipStreamWaitEvent(st, c->ev_pset[k], 0));
    if (c->carry_seed && c->chans_armed) HIPCHK(hipStreamWaitEvent(st, c->ev_chans, 0));
    const size_t al = (size_t)c->pl.rates | (size_t)c->pl.bws | (size_t)c->pl.nb | (size_t)c->pl.fl;
    const int vec4 = (T & 3) == 0 && (al & 15) == 0 && (((size_t)c->pl.fl) & 3) == 0;
    auto plan = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3((unsigned)((c->n_streams + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, c->pl.rule, c->pl.rates, c->pl.bws, T,
                       c->n_streams, c->d_carry, c->carry_seed ? (const lc3d_chan*)c->d_chans : (const lc3d_chan*)nullptr, c->d_pfsz[k], c->d_pbw[k], c->pl.nb, c->pl.fl,
                       c->d_pend[k], vec4, ragged...); };
    /* ragged: the clamped counts, and for slotted output the table of slots in this set's offset table (a packed call's scan fills it below) */
    if (c->rag) { plan(lc3_enc_plan_rates_kernel_rag, c->counts, c->d_cnt, c->pk.on ? (long long*)nullptr : c->d_poff[k], c->pl.stride); if (!c->pk.on) c->pk.tab = c->d_poff[k]; }
    else plan(lc3_enc_plan_rates_kernel);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_plan, st)); c->plan_armed = 1;
    c->carry_seed = 0; c->pl.pending = 0;
    /* packed output: the offsets behind the sizes, on the same stream (the writers, on whichever stream, are behind this one: bw_to, ev_scan) */
    if (c->pk.on && pack_scan(c, st, T, k, c->pl.rates || c->rag ? c->d_pfsz[k] : nullptr, c->d_pend[k], c->pl.fl != nullptr, c->pl.nb != nullptr)) return 1;
    return 0;
}
/* Per-frame rates and / or bandwidths in device memory, as PCM and output: the plan kernel turns them into the words the per-frame kernels read (it runs
 * where the first of those kernels runs: bw_to), the call takes the path lc3hip_encode takes with the same words from the host, and the tail kernel
 * configures every stream on s behind it.  Nothing is read back, and the host waits only where a set of plan buffers has to grow. */
extern "C" int lc3hip_encode_rates_device(void* ctx, const void* pcm, int bitdepth, int n_frames, void* out, int out_stride, const int32_t* rates_dev,
                                          const int32_t* bws_dev, const lc3d_rate_rule* rule, int32_t* num_bytes_dev, uint8_t* flags_dev, int clear_resets,
                                          void* hip_stream, int sync)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (!c->d_etab || (bws_dev && c->big)) return 1;
    if (c->wk.calls && work_poison_all(&c->wk)) return 1;
    if (!hip_stream && !c->stream) HIPCHK(hipStreamCreate(&c->stream));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (!c->ev_plan) {
        HIPCHK(hipEventCreateWithFlags(&c->ev_plan, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_pset_prev, hipEventDisableTiming));
        for (int i = 0; i < LC3D_SETS; i++) HIPCHK(hipEventCreateWithFlags(&c->ev_pset[i], hipEventDisableTiming));
        if (!c->ev_bwcp) HIPCHK(hipEventCreateWithFlags(&c->ev_bwcp, hipEventDisableTiming));
        c->carry_seed = 1;
    }
    if (grow_once(&c->d_carry, sizeof(int4) * (size_t)c->n_streams)) return 1;      /* outside the block above: a call after a failed allocation tries again */
    for (int i = 0; i < LC3D_SETS; i++) if (grow_once(&c->d_pend[i], sizeof(int4) * (size_t)c->n_streams, false, &c->wk)) return 1;
    /* an earlier call that did not wait may still read the smaller sets: growing them waits for the device, once (the first allocation does not) */
    const size_t fb = sizeof(uint16_t) * (size_t)c->n_streams * n_frames;
    lc3hip_buf b[2 * LC3D_SETS];
    for (int i = 0; i < LC3D_SETS; i++) { b[2 * i] = {(void**)&c->d_pfsz[i], fb, false}; b[2 * i + 1] = {(void**)&c->d_pbw[i], fb, false}; }
    if (grow_group(&c->pset_frames, (size_t)n_frames, b, 2 * LC3D_SETS, true, &c->wk)) return 1;
    /* Ragged (lc3hip_set_frame_counts): the call of this function with the _rag kernels.  Its plan kernel always writes sizes - the carried ones where the caller
     * gave no rates - and an offset table (slotted output: every frame's slot), on s in front of everything else of the call (bw_to below): every other kernel reads
     * the clamped counts it leaves, and on the pipelined path (enc_launch: long calls without rates in the standard layout) the side streams fork from s behind it.
     * Either path ends every overlap (enc_one_wave, enc_pipelined), and the call after it forks from s again. */
    const int rag = c->counts != nullptr;
    if (rag && !c->pk.on && pk_tables(c, (size_t)c->n_streams * n_frames)) return 1;
    c->rag = rag ? (rates_dev ? 1 : 2) : 0; c->pl.stride = out_stride;
    struct rag_off { lc3hip_ctx* c; ~rag_off() { if (c->rag && !c->pk.on) c->pk.tab = nullptr; c->rag = 0; } } rag_end = {c};      /* however the call ends */
    const int k = c->pset;
    c->pl.pending = 1; c->pl.k = k; c->pl.T = n_frames; c->pl.rates = rates_dev; c->pl.bws = bws_dev; c->pl.nb = num_bytes_dev; c->pl.fl = flags_dev; c->pl.rule = *rule;
    c->bw_on = nullptr;
    if (c->chans_armed) HIPCHK(hipStreamWaitEvent(s, c->ev_chans, 0));
    /* behind the batch's last call when that went to another stream (its work there ends on it: writer, rate chain), as a stream-lifecycle call is */
    if (c->last_stream && c->last_stream != s) { HIPCHK(hipEventRecord(c->ev_pset_prev, c->last_stream)); HIPCHK(hipStreamWaitEvent(s, c->ev_pset_prev, 0)); }
    HIPCHK(hipEventRecord(c->ev0, s));
    if ((rates_dev || rag) && bw_to(c, s)) return 1;                         /* the one-wave kernels on s read the sizes: the plan kernel in front of them */
    if (enc_launch(c, pcm, bitdepth, n_frames, (uint8_t*)out, out_stride, s, nullptr, n_frames, 0, true, rates_dev || rag ? c->d_pfsz[k] : nullptr,
                   bws_dev ? c->d_pbw[k] : nullptr)) return 1;
    if (c->pl.pending) return 1;                                             /* every path reads the words */
    auto tail = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3((unsigned)((c->ncs + WAVE - 1) / WAVE)), dim3(WAVE), 0, s, (const int4*)c->d_pend[k], (const lc3d_chan*)c->d_etab,
                       c->d_chans, c->channels, c->ncs, rule->dms, rates_dev ? 1 : 0, ragged...); };
    if (rag) tail(lc3_enc_rates_tail_kernel_rag, (const int32_t*)c->d_cnt); else tail(lc3_enc_rates_tail_kernel);
    HIPCHK(hipGetLastError());
    if (placed_mark(c->plo, c->plcap, c->channels, c->N, (long long)c->n_streams * n_frames, flags_dev, LC3D_ENC_FL_PCM_PLACE, s)) return 1;
    if (rag && flags_dev) {      /* last: an absent frame's flags are exactly LC3D_ENC_FL_ABSENT, whatever the scan and the mark above put beside it */
        const long long n = (long long)c->n_streams * n_frames;
        LC3_LAUNCH(lc3_enc_absent_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const int32_t*)c->d_cnt, n_frames, n, flags_dev);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(c->ev1, s));
    HIPCHK(hipEventRecord(c->ev_pset[k], s)); c->pset_armed[k] = 1; c->pset = (k + 1) % LC3D_SETS;
    /* the configuration the tail kernel wrote: later calls on other streams wait for it (as for lc3hip_upload_chans_async); a call that overlaps this one may
     * do so only where the tail changed the bandwidth words alone */
    if (!c->ev_chans) HIPCHK(hipEventCreateWithFlags(&c->ev_chans, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_chans, s)); c->chans_armed = 1;
    c->cfg_fresh = (rates_dev || clear_resets) ? 2 : 1;
    /* what the launch decisions know of the configuration until the host reads it back: with rates any stream may now have attack handling, and channel
     * frames of any size of the table */
    if (rates_dev) { c->any_attack |= c->etab_attack; c->max_nbytes = c->etab_max; c->min_nbytes = 1; }
    if (c->opt.check_ready && c->ev_ours) { HIPCHK(hipEventRecord(c->ev_ours, s)); c->ours_armed = 1; }
    c->last_stream = s;
    if (sync) SYNC_TIMED(c, s);
    return 0;
}
/* Packed output: the call of lc3hip_encode_rates_device (rates_dev or bws_dev given) or of lc3hip_encode with device pointers (neither), with the scan of
 * the call's frame sizes in front of its writers and the _pk kernels writing each frame at its offset.  The tables grow as the plan sets do: an earlier
 * call that did not wait may still read the smaller ones, so growing them waits for the device, once. */
extern "C" int lc3hip_encode_packed(void* ctx, const void* pcm, int bitdepth, int n_frames, const int32_t* rates_dev, const int32_t* bws_dev,
                                    const lc3d_rate_rule* rule, int order, void* out, long long capacity, long long* offsets_dev, long long* total_dev,
                                    int32_t* num_bytes_dev, uint8_t* flags_dev, int clear_resets, void* hip_stream, int sync)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    /* one table of offsets per slot and, in one buffer, a slot of tile sums for each; an earlier call that did not wait may still read the smaller tables, so
     * growing them waits for the device, once (the first allocation does not) */
    if (pk_tables(c, (size_t)c->n_streams * n_frames)) return 1;
    if (!c->ev_scan) HIPCHK(hipEventCreateWithFlags(&c->ev_scan, hipEventDisableTiming));
    c->pk.on = 1; c->pk.order = order; c->pk.cap = capacity; c->pk.offs = offsets_dev; c->pk.total = total_dev; c->pk.nb = num_bytes_dev; c->pk.fl = flags_dev;
    c->pk.tab = nullptr;
    int rc;
    if (rates_dev || bws_dev || c->counts)      /* (ragged with neither: the plan kernel still runs, on the carried sizes) */
        rc = lc3hip_encode_rates_device(ctx, pcm, bitdepth, n_frames, out, 0, rates_dev, bws_dev, rule, num_bytes_dev, flags_dev, clear_resets, hip_stream, sync);
    else
        rc = lc3hip_encode(ctx, pcm, 1, bitdepth, n_frames, out, 0, 1, hip_stream, sync, nullptr, nullptr, nullptr);
    c->pk.on = 0; c->pk.tab = nullptr;
    return rc;
}
/* waits for the batch's last call and copies the configuration of every channel-stream to chans[ncs] (after lc3hip_encode_rates_device) */
extern "C" int lc3hip_download_chans(void* ctx, lc3d_chan* chans)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (c->last_stream) HIPCHK(hipStreamSynchronize(c->last_stream));
    if (c->chans_armed) HIPCHK(hipEventSynchronize(c->ev_chans));
    HIPCHK(hipMemcpy(chans, c->d_chans, sizeof(lc3d_chan) * (size_t)c->ncs, hipMemcpyDeviceToHost));
    return chans_host_side(c, chans, 0, c->ncs);
}

/* waits for the batch's last call (a call made with sync = 0) */
extern "C" int lc3hip_wait(void* ctx)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (c->last_stream) HIPCHK(hipStreamSynchronize(c->last_stream));
    return 0;
}

/* status bits of the last call, [channel-stream][frame] (n = ncs * frames of that call), to host memory */
extern "C" int lc3hip_last_status(void* ctx, uint8_t* status_host, int n)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (n > c->ncs * c->status_frames) n = c->ncs * c->status_frames;
    if (c->last_stream) HIPCHK(hipStreamSynchronize(c->last_stream));
    if (n > 0) HIPCHK(hipMemcpy(status_host, c->d_status, (size_t)n, hipMemcpyDeviceToHost));
    return n;
}

/* the per-frame records of the last call of the pipelined path (FR_* in lc3_plan.h: scale factors, SNS indices, bandwidth, LTPF and TNS parameters, gain floor,
 * the rate kernel's four words), [channel-stream][frame][FR_WORDS] to host memory: stage-level parity tests of the product path read them */
extern "C" int lc3hip_last_records(void* ctx, float* rec_host, int max_words)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    if (!c || !c->last_frec) return 0;
    HIPCHK(hipSetDevice(c->device));
    if (c->last_stream) HIPCHK(hipStreamSynchronize(c->last_stream));
    long long n = (long long)c->ncs * c->last_frec_frames * FR_WORDS;
    if (n > max_words) n = max_words;
    if (n > 0) HIPCHK(hipMemcpy(rec_host, c->last_frec, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return (int)n;
}

/* checkpoint / resume: the cross-frame state of every channel-stream (LC3D_STATE_WORDS words each, the layout of lc3_plan.h) as one host
 * array; everything else a batch holds is derived from its configuration.  Both wait for the last call to finish. */
extern "C" size_t lc3hip_state_bytes(void* ctx) { lc3hip_ctx* c = (lc3hip_ctx*)ctx; return c ? sizeof(float) * (size_t)c->state_words * (size_t)c->ncs : 0; }
extern "C" int lc3hip_get_state(void* ctx, void* host, size_t bytes)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    if (!c || !host || bytes != lc3hip_state_bytes(ctx)) return 1;
    HIPCHK(hipSetDevice(c->device));
    if (c->last_stream) HIPCHK(hipStreamSynchronize(c->last_stream));
    HIPCHK(hipMemcpy(host, c->d_state, bytes, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int lc3hip_set_state(void* ctx, const void* host, size_t bytes)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    if (!c || !host || bytes != lc3hip_state_bytes(ctx)) return 1;
    HIPCHK(hipSetDevice(c->device));
    if (c->last_stream) HIPCHK(hipStreamSynchronize(c->last_stream));
    HIPCHK(hipMemcpy(c->d_state, host, bytes, hipMemcpyHostToDevice));
    c->ahead_ok = 0;                       /* the MDCT memory is in the state, not in a previous call's hand-over */
    return 0;
}

extern "C" int lc3hip_stream_state(void* ctx, int mode, const int* streams, int n, const lc3d_chan* cfg, void* blob, int blob_on_device, const uint32_t* hdr,
                                   uint8_t* status, void* hip_stream, int sync)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (!hip_stream && !c->stream) HIPCHK(hipStreamCreate(&c->stream));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    /* behind the batch's last call: on its stream the writer, and the rate chain of a pipelined call, whose last rate kernel has written the MDCT memory
     * into the state (the side streams carry nothing of that call's state work beyond it); behind a configuration copy queued on another stream */
    if (c->chans_armed) HIPCHK(hipStreamWaitEvent(s, c->ev_chans, 0));
    if (ss_run(&c->ss, s, c->last_stream, mode, c->d_state, c->channels, streams, n, cfg, (int)sizeof(lc3d_chan), c->d_chans, blob, blob_on_device, hdr, status, sync)) return 1;
    /* every later call waits for this one on its own stream (ev_chans: encode, the configuration copies); the next call does not read the MDCT memory from a
     * hand-over, and starts its side streams behind this call */
    if (!c->ev_chans) HIPCHK(hipEventCreateWithFlags(&c->ev_chans, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_chans, s)); c->chans_armed = 1;
    c->ahead_ok = 0;
    c->last_stream = s;
    if (cfg) c->carry_seed = 1;
    return cfg ? chans_host_side_list(c, cfg, 0, n * c->channels, streams) : 0;
}

/* records the pair: every later call reads it (enc_launch, launch_resample); nothing is queued */
extern "C" int lc3hip_set_pcm_placement(void* ctx, const long long* offsets_dev, long long capacity)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    if (!c || capacity < 0) return 1;
    c->plo = offsets_dev; c->plcap = offsets_dev ? capacity : 0;
    return 0;
}
/* records the pointer: lc3hip_encode_rates_device and lc3hip_encode_packed read it when they are called, their plan kernel reads the array when it runs */
extern "C" int lc3hip_set_frame_counts(void* ctx, const int32_t* counts_dev)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    if (!c) return 1;
    c->counts = counts_dev;
    return 0;
}
extern "C" int lc3hip_set_input_ready(void* ctx, int ready)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    if (!c) return 1;
    c->input_ready = ready != 0; c->ahead_ok = 0;
    return 0;
}

extern "C" float lc3hip_last_ms(void* ctx)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    float ms = 0;
    if (hipEventSynchronize(c->ev1) == hipSuccess && hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->last_ms = ms;
    return c->last_ms;
}

extern "C" int lc3hip_work_buffer(void* ctx, int i, const char** name, void** ptr, size_t* bytes, int* elem) { return ctx ? work_buffer_at(&((lc3hip_ctx*)ctx)->wk, i, name, ptr, bytes, elem) : 1; }

extern "C" int lc3hip_destroy(void* ctx)
{
    lc3hip_ctx* c = (lc3hip_ctx*)ctx;
    if (!c) return 0;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    void* bufs[] = {c->d_plan, c->d_chans, c->d_state, c->d_pcm, c->d_out, c->d_trace, c->d_etab, c->d_carry, c->d_pbsum, c->hp_dpcm[0], c->hp_dpcm[1], c->d_cnt};
    for (void* p : bufs) if (p) hipFree(p);
    for (int i = 0; i < LC3D_SETS; i++) {      /* what a set holds: hand-over buffers, plan buffers */
        void* set[] = {c->d_dumpv[i], c->d_statusv[i], c->d_y12[i], c->d_spec[i], c->d_frec[i], c->d_pfsz[i], c->d_pbw[i], c->d_pend[i]};
        for (void* p : set) if (p) hipFree(p);
        if (c->ev_pset[i]) hipEventDestroy(c->ev_pset[i]);
    }
    for (int i = 0; i < LC3D_SETS + 1; i++) { if (c->d_xnext[i]) hipFree(c->d_xnext[i]); if (c->d_poff[i]) hipFree(c->d_poff[i]); }
    free(c->h_attack); free(c->h_nb);
    if (c->h_chans) hipHostFree(c->h_chans);
    if (c->ev_chans) hipEventDestroy(c->ev_chans);
    ss_free(&c->ss);
    stage_free(&c->fsz); stage_free(&c->bw);
    if (c->ev_bwcp) hipEventDestroy(c->ev_bwcp);
    if (c->ev_plan) { hipEventDestroy(c->ev_plan); hipEventDestroy(c->ev_pset_prev); }
    if (c->ev_scan) hipEventDestroy(c->ev_scan);
    for (int i = 0; i < 2; i++) { if (c->hp_pin_in[i]) hipHostFree(c->hp_pin_in[i]); if (c->ev_h2d[i]) hipEventDestroy(c->ev_h2d[i]); if (c->ev_k[i]) hipEventDestroy(c->ev_k[i]); }
    if (c->s_h2d) hipStreamDestroy(c->s_h2d);
    if (c->s_pre) { if (c->s_pit != c->s_pre) { hipStreamDestroy(c->s_pit); hipStreamDestroy(c->s_ln); } hipStreamDestroy(c->s_pre); hipStreamDestroy(c->s_fr); for (int i = 0; i < 2; i++) { if (c->s_pk[i]) hipStreamDestroy(c->s_pk[i]); hipEventDestroy(c->ev_pk[i]); } hipEventDestroy(c->ev_rate);
                    for (int i = 0; i < LC3D_MAX_RUNS; i++) { hipEventDestroy(c->ev_h[i]); hipEventDestroy(c->ev_m[i]); hipEventDestroy(c->ev_v[i]); } hipEventDestroy(c->ev_fork); for (int i = 0; i < LC3D_SETS; i++) hipEventDestroy(c->ev_done[i]);
                    for (int i = 0; i < LC3D_MAX_RUNS; i++) { hipEventDestroy(c->ev_p[i]); hipEventDestroy(c->ev_f[i]); } }
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->ev_ours) { hipEventDestroy(c->ev_ours); hipEventDestroy(c->ev_now); }
    if (c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
    free(c);
    return 0;
}
/* ---- decoder shim ---- */
#ifndef DEC_SETS
#define DEC_SETS 3                      /* sets of hand-over buffers (records, spectrum rows) under the decoder's input-ready promise: the parser of call k + 2 may write while call k is synthesised */
#endif
struct lc3hip_dctx {
    lc3hip_opts opt; work_set wk;
    int device, ncs, n_streams, channels, N, big;
    lc3d_plan* d_plan; lc3d_dchan* d_chans; float* d_state;
    uint8_t* d_in; size_t in_cap; void* d_pcm; size_t pcm_cap; uint8_t* d_bfi; size_t bfi_cap;
    lc3d_dchan* d_tab; int tab_n; uint16_t* d_sizes; size_t sizes_cap;          /* per-frame sizes: configuration per channel byte count, effective size per stream-frame */
    uint8_t* d_inval; size_t inval_cap;                              /* per-frame sizes from device memory: the frames lost because their size or flag is invalid */
    lc3d_dec_trace* d_trace; size_t trace_cap; uint8_t* d_status; size_t status_cap;
    int* d_rec; float* d_ws; float* d_ov; size_t hand_cap; int max_nbytes; int* h_nbytes;
    hipStream_t stream, last_stream; hipEvent_t ev0, ev1; float last_ms;
    /* lc3hip_dec_set_input_ready: the parse kernel of a call runs on a stream of its own beside the transform and synthesis of the call before; a
     * second set of hand-over buffers (records, spectrum rows), alternating */
    const long long* plo; long long plcap;         /* lc3hip_dec_set_pcm_placement */
    const int32_t* counts; int32_t* d_cnt;         /* lc3hip_dec_set_frame_counts: the caller's per-stream frame counts (null: off), and the clamped copy [n_streams] the ragged kernels of a call read */
    int input_ready, set; int* d_recx[DEC_SETS - 1]; float* d_wsx[DEC_SETS - 1]; size_t handx_cap; hipStream_t s_par, s_plc; hipEvent_t ev_par[DEC_SETS], ev_free[DEC_SETS], ev_plc; int free_armed[DEC_SETS];
    /* the end of the last ordered call (bad-frame flags, per-frame sizes, status, host pointers) under the promise: the next parse-ahead waits for it */
    hipEvent_t ev_ord; int ord_pending;
    lc3hip_ss ss;                                   /* the fresh-row template, lc3hip_dec_stream_state */
};
/* the decoder's work buffers.  Not here: d_state and d_chans (a later call reads what an earlier one wrote), the lifecycle staging, d_plan, d_tab and the template */
static const work_buf dec_work[] = {
    WORK(lc3hip_dctx, d_in, 1, LC3HIP_ELEM_U8, c->in_cap),
    WORK(lc3hip_dctx, d_pcm, 1, LC3HIP_ELEM_U8, c->pcm_cap),
    WORK(lc3hip_dctx, d_bfi, 1, LC3HIP_ELEM_U8, c->bfi_cap),
    WORK(lc3hip_dctx, d_sizes, 1, LC3HIP_ELEM_U16, c->sizes_cap),
    WORK(lc3hip_dctx, d_inval, 1, LC3HIP_ELEM_U8, c->inval_cap),
    WORK(lc3hip_dctx, d_trace, 1, LC3HIP_ELEM_U8, c->trace_cap),
    WORK(lc3hip_dctx, d_status, 1, LC3HIP_ELEM_U8, c->status_cap),
    WORK(lc3hip_dctx, d_rec, 1, LC3HIP_ELEM_I32, c->hand_cap * PR_WORDS * sizeof(int)),
    WORK(lc3hip_dctx, d_ws, 1, LC3HIP_ELEM_F32, c->hand_cap * WS_ROW(c->N) * sizeof(float)),
    WORK(lc3hip_dctx, d_ov, 1, LC3HIP_ELEM_F32, c->hand_cap * (c->big ? OV_ROW_BIG : OV_ROW_STD) * sizeof(float)),
    WORK(lc3hip_dctx, d_recx, DEC_SETS - 1, LC3HIP_ELEM_I32, c->handx_cap * PR_WORDS * sizeof(int)),
    WORK(lc3hip_dctx, d_wsx, DEC_SETS - 1, LC3HIP_ELEM_F32, c->handx_cap * WS_ROW(c->N) * sizeof(float)),
    WORK(lc3hip_dctx, d_cnt, 1, LC3HIP_ELEM_I32, sizeof(int32_t) * (size_t)c->n_streams),
};
extern "C" int lc3hip_dec_work_buffer(void* ctx, int i, const char** name, void** ptr, size_t* bytes, int* elem) { return ctx ? work_buffer_at(&((lc3hip_dctx*)ctx)->wk, i, name, ptr, bytes, elem) : 1; }
static int dec_side_streams(lc3hip_dctx* c)                       /* the parse-ahead stream, the concealment stream and their events, created once */
{
    if (c->s_par) return 0;
    HIPCHK(hipStreamCreateWithFlags(&c->s_par, hipStreamNonBlocking));
    for (int i = 0; i < DEC_SETS; i++) { HIPCHK(hipEventCreateWithFlags(&c->ev_par[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_free[i], hipEventDisableTiming)); }
    HIPCHK(hipStreamCreateWithFlags(&c->s_plc, hipStreamNonBlocking)); HIPCHK(hipEventCreateWithFlags(&c->ev_plc, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_ord, hipEventDisableTiming));
    return 0;
}
extern "C" int lc3hip_dec_destroy(void* ctx);
extern "C" int lc3hip_dec_create(void** out_ctx, const lc3d_plan* plan, const float* tmpl, int n_streams, int device)
{
    int ndev = 0;
    *out_ctx = nullptr;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { fprintf(stderr, "lc3plus_hip: no HIP device available (this engine has no CPU fallback)\n"); return 1; }
    lc3hip_dctx* c = (lc3hip_dctx*)calloc(1, sizeof *c);
    if (!c) return 1;
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    c->device = device;
    HIPCHK_OR(hipSetDevice(device), free(c));
    c->n_streams = n_streams; c->channels = plan->channels; c->ncs = n_streams * plan->channels; c->N = plan->N;
    c->big = LC3D_LAYOUT_BIG(plan->N, plan->la);
    read_opts(&c->opt);
    HIPCHK_OR(hipMalloc((void**)&c->d_plan, sizeof(lc3d_plan)), lc3hip_dec_destroy(c));
    HIPCHK_OR(hipMemcpy(c->d_plan, plan, sizeof(lc3d_plan), hipMemcpyHostToDevice), lc3hip_dec_destroy(c));
    HIPCHK_OR(hipMalloc((void**)&c->d_chans, sizeof(lc3d_dchan) * c->ncs), lc3hip_dec_destroy(c));
    HIPCHK_OR(hipMalloc((void**)&c->d_state, sizeof(float) * DST_WORDS * (size_t)c->ncs), lc3hip_dec_destroy(c));
    HIPCHK_OR(hipMalloc((void**)&c->d_cnt, sizeof(int32_t) * (size_t)n_streams), lc3hip_dec_destroy(c));
    c->wk = {c, dec_work, (int)(sizeof dec_work / sizeof *dec_work), c->opt.poison_work, c->opt.poison_calls};
    if (c->wk.set && work_poison_all(&c->wk)) { lc3hip_dec_destroy(c); return 1; }      /* what exists by now: the counts */
    if (ss_init(&c->ss, c->device, c->d_state, DST_WORDS, c->ncs, tmpl)) { lc3hip_dec_destroy(c); return 1; }
    HIPCHK_OR(hipStreamCreate(&c->stream), lc3hip_dec_destroy(c));
    HIPCHK_OR(hipEventCreate(&c->ev0), lc3hip_dec_destroy(c)); HIPCHK_OR(hipEventCreate(&c->ev1), lc3hip_dec_destroy(c));
    *out_ctx = c;
    return 0;
}
/* the largest frame of the batch selects the parse kernel's staging: kept exact when sizes shrink again.  Channel-streams first ... first + count - 1, or with
 * list the channels of streams list[0 .. count / channels - 1] */
static int dec_note_nbytes(lc3hip_dctx* c, const lc3d_dchan* chans, int first, int count, const int* list)
{
    if (!c->h_nbytes) { c->h_nbytes = (int*)calloc((size_t)c->ncs, sizeof(int)); if (!c->h_nbytes) return 1; }
    for (int i = 0; i < count; i++) c->h_nbytes[list ? list[i / c->channels] * c->channels + i % c->channels : first + i] = chans[i].nbytes;
    c->max_nbytes = 0;
    for (int i = 0; i < c->ncs; i++) if (c->h_nbytes[i] > c->max_nbytes) c->max_nbytes = c->h_nbytes[i];
    return 0;
}
extern "C" int lc3hip_dec_upload_chans(void* ctx, const lc3d_dchan* chans, int first, int count)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (c->last_stream) { HIPCHK(hipStreamSynchronize(c->last_stream)); c->last_stream = nullptr; }
    HIPCHK(hipMemcpy(c->d_chans + first, chans, sizeof(lc3d_dchan) * count, hipMemcpyHostToDevice));
    return dec_note_nbytes(c, chans, first, count, nullptr);
}
extern "C" int lc3hip_dec_upload_table(void* ctx, const lc3d_dchan* tab, int n)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (replace(&c->d_tab, sizeof(lc3d_dchan) * (size_t)n)) return 1;      /* as the encoder's table */
    HIPCHK(hipMemcpy(c->d_tab, tab, sizeof(lc3d_dchan) * (size_t)n, hipMemcpyHostToDevice));
    c->tab_n = n;
    return 0;
}
extern "C" int lc3hip_dec_wait(void* ctx)            /* as lc3hip_wait */
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (c->last_stream) HIPCHK(hipStreamSynchronize(c->last_stream));
    return 0;
}
extern "C" int lc3hip_dec_download_chans(void* ctx, lc3d_dchan* chans)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    if (c->last_stream) { HIPCHK(hipStreamSynchronize(c->last_stream)); c->last_stream = nullptr; }
    HIPCHK(hipMemcpy(chans, c->d_chans, sizeof(lc3d_dchan) * c->ncs, hipMemcpyDeviceToHost));
    return dec_note_nbytes(c, chans, 0, c->ncs, nullptr);
}
/* one call of dec_decode: its arguments, and what the functions it is cut into hand to each other.
 * nb_dev: per-frame sizes in device memory (lc3hip_dec_decode_dsizes) - with bfi_dev (or null) and status_dev (or null), all device pointers like frames and pcm */
struct dec_call {
    const void* frames; int frames_on_device, in_stride; const uint8_t* bfi_host; const uint16_t* sizes_host; int sizes_max_nbytes, n_frames; void* pcm; int pcm_on_device, bps;
    uint8_t* status_host; int sync; void* trace_host; const int32_t* nb_dev; const uint8_t* bfi_dev; uint8_t* status_dev;
    const long long* offs_dev;      /* frames packed (lc3hip_dec_decode_packed): in_stride is then the largest frame */
    long long cap;
    hipStream_t s; const int32_t* cnt;
    const uint8_t* din; void* dpcm; const uint8_t* dbfi; const uint16_t* dsizes; lc3d_dec_trace* dtr; uint8_t* dst; size_t pcm_bytes;      /* dec_stage: what the kernels read and write */
    bool ahead; int* rec_w; float* ws_w;                                                                                               /* dec_stage: the set of hand-over buffers the parser writes */
    int max_nb, nw_max, wpg; size_t per_wave;                                                                                          /* dec_parse_lds */
};
/* staging host arrays: what the call brings in host memory goes to the device on s, and every buffer of the call is sized.  The host-array buffers (d_in, d_pcm,
 * d_bfi, d_sizes, d_trace, d_status) grow without a wait of their own: a call that uses one returns when its work is done, and hipFree waits for the device's
 * pending work before it releases anything. */
static int dec_stage(lc3hip_dctx* c, dec_call* q)
{
    hipStream_t s = q->s;
    const int n_frames = q->n_frames;
    const size_t in_bytes = (size_t)c->n_streams * n_frames * q->in_stride;
    q->pcm_bytes = (size_t)c->ncs * n_frames * c->N * (size_t)lc3d_pcm_elem_bytes(q->bps);
    q->din = (const uint8_t*)q->frames; q->dpcm = q->pcm;
    /* a device buffer of `bytes` for a host array of the call, and the array (if any: h) copied into it on s */
    auto up = [&](auto** d, size_t* cap, const void* h, size_t bytes) -> int { if (grow(d, cap, bytes, bytes, false, &c->wk)) return 1; if (h) HIPCHK(hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, s)); return 0; };
    const size_t fb = (size_t)c->n_streams * n_frames;            /* a byte per stream-frame */
    if (!q->frames_on_device) { if (up(&c->d_in, &c->in_cap, q->frames, in_bytes)) return 1; q->din = c->d_in; }
    if (!q->pcm_on_device) { if (up(&c->d_pcm, &c->pcm_cap, nullptr, q->pcm_bytes)) return 1; q->dpcm = c->d_pcm; }
    if (q->bfi_host) { if (up(&c->d_bfi, &c->bfi_cap, q->bfi_host, fb)) return 1; q->dbfi = c->d_bfi; }
    if (q->sizes_host) {                                            /* per-frame sizes: the host merged the lost frames into bfi_host, so this call is ordered */
        if (!q->bfi_host || !c->d_tab || up(&c->d_sizes, &c->sizes_cap, q->sizes_host, sizeof(uint16_t) * fb)) return 1;
        q->dsizes = c->d_sizes;
    }
    if (q->trace_host) {
        const size_t tb = sizeof(lc3d_dec_trace) * (size_t)c->ncs * n_frames;
        if (up(&c->d_trace, &c->trace_cap, nullptr, tb)) return 1;
        HIPCHK(hipMemsetAsync(c->d_trace, 0, tb, s));
        q->dtr = c->d_trace;
    }
    if (q->status_host) { if (up(&c->d_status, &c->status_cap, nullptr, fb)) return 1; q->dst = c->d_status; }
    if (q->nb_dev) {                                                /* sizes and flags from device memory: the plan kernel fills d_sizes / d_bfi / d_inval */
        if (!c->d_tab) return 1;
        /* a smaller buffer of an earlier call may still be read (calls of this kind do not wait): growing it waits for the device; the first allocation does not.
         * (Three capacities - the host-array calls above grow two of the buffers on their own: each that grows waits, and behind the first wait the device is idle.) */
        if (grow(&c->d_sizes, &c->sizes_cap, sizeof(uint16_t) * fb, sizeof(uint16_t) * fb, true, &c->wk) || grow(&c->d_bfi, &c->bfi_cap, fb, fb, true, &c->wk) || grow(&c->d_inval, &c->inval_cap, fb, fb, true, &c->wk)) return 1;
        q->dsizes = c->d_sizes; q->dbfi = c->d_bfi; q->dst = q->status_dev;
    }
    const size_t cf = (size_t)c->ncs * n_frames;
    /* hand-over buffers between the two kernels: records and spectrum rows of every channel-frame of this call; an earlier call that did not wait may still read them (not on the first call) */
    const lc3hip_buf hand[] = {{(void**)&c->d_rec, cf * PR_WORDS * sizeof(int), false}, {(void**)&c->d_ws, cf * WS_ROW(c->N) * sizeof(float), false},
                               {(void**)&c->d_ov, cf * (c->big ? OV_ROW_BIG : OV_ROW_STD) * sizeof(float), false}};
    if (grow_group(&c->hand_cap, cf, hand, 3, true, &c->wk)) return 1;
    /* Under the input-ready promise (the frames of a call are complete on the device when the call is made) the parse kernel - stateless: a frame's
     * record and spectrum row depend on that frame's bytes only - does not wait for what is queued on s: it runs on its own stream into the other set of
     * hand-over buffers while the concealment bookkeeping, transform and synthesis of the call before (the stateful part, in order on s) read theirs. */
    q->ahead = c->input_ready && q->frames_on_device && q->pcm_on_device && !q->bfi_host && !q->trace_host && !q->status_host && !q->nb_dev;
    q->rec_w = c->d_rec; q->ws_w = c->d_ws;
    if (q->ahead) {
        if (dec_side_streams(c)) return 1;
        lc3hip_buf handx[2 * (DEC_SETS - 1)];      /* the other sets: calls in flight read them, so growing them waits for the device (not before the first allocation: nothing reads buffers that do not exist) */
        for (int i = 0; i < DEC_SETS - 1; i++) {
            handx[2 * i] = {(void**)&c->d_recx[i], cf * PR_WORDS * sizeof(int), false};
            handx[2 * i + 1] = {(void**)&c->d_wsx[i], cf * WS_ROW(c->N) * sizeof(float), false};
        }
        if (grow_group(&c->handx_cap, cf, handx, 2 * (DEC_SETS - 1), true, &c->wk)) return 1;
        if (c->set) { q->rec_w = c->d_recx[c->set - 1]; q->ws_w = c->d_wsx[c->set - 1]; }
    }
    return 0;
}
/* the parser's LDS: how many words of a frame a lane stages, and how many waves share a workgroup's tables */
static int dec_parse_lds(lc3hip_dctx* c, dec_call* q)
{
    /* frames of up to 128 bytes are staged in LDS; larger ones would cut the waves per workgroup and are read from global memory */
    /* (per-frame sizes: the largest channel frame of the call that is not lost - lost frames stage nothing; sizes in device memory are not seen by the
     * host: the bound it knows, a channel's share of in_stride up to the geometry's largest channel frame - a tight in_stride keeps the staged parser) */
    const int ch_share = (q->in_stride + c->channels - 1) / c->channels;
    q->max_nb = q->nb_dev ? (ch_share < c->tab_n - 1 ? ch_share : c->tab_n - 1) : q->dsizes ? q->sizes_max_nbytes : c->max_nbytes;
    q->nw_max = q->max_nb > 128 ? 0 : q->max_nb > 0 ? (q->max_nb + 3) / 4 : 1;
    const int nlw = (WS_ROW(c->N) / 2 + 31) / 32;                          /* >= (ylen / 2 + 31) / 32 of the plan */
    q->per_wave = (size_t)(q->nw_max + nlw) * WAVE * sizeof(unsigned);
    q->wpg = (int)((64 * 1024 - sizeof(ParseLds)) / q->per_wave);          /* waves per workgroup: they share the model tables */
    if (q->wpg > 4) q->wpg = 4;
    if (q->wpg < 1) { fprintf(stderr, "lc3plus_hip: frame of %d bytes exceeds the parse kernel's LDS staging\n", q->max_nb); return 1; }
    return 0;
}
/* the plan kernel of a call with sizes in device memory, on s: the sizes, loss flags and invalid flags the other kernels read; ragged, also the clamped counts */
static int dec_plan(lc3hip_dctx* c, const dec_call* q)
{
    const long long n = (long long)c->n_streams * q->n_frames;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    auto packed = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, grid, block, 0, q->s, q->nb_dev, q->offs_dev, q->bfi_dev, c->d_tab, c->tab_n, c->channels, q->cap, q->in_stride, n, c->d_sizes, c->d_bfi, c->d_inval, ragged...); };
    auto sizes = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, grid, block, 0, q->s, q->nb_dev, q->bfi_dev, c->d_tab, c->tab_n, c->channels, q->in_stride, n, c->d_sizes, c->d_bfi, c->d_inval, ragged...); };
    if (q->offs_dev) { if (q->cnt) packed(lc3_dec_plan_packed_kernel_rag, c->counts, q->n_frames, c->d_cnt); else packed(lc3_dec_plan_packed_kernel); }
    else if (q->cnt) sizes(lc3_dec_plan_sizes_kernel_rag, c->counts, q->n_frames, c->d_cnt);
    else sizes(lc3_dec_plan_sizes_kernel);
    HIPCHK(hipGetLastError());
    return 0;
}
/* parse: one stream-frame per lane, on sp */
static int dec_parse(lc3hip_dctx* c, const dec_call* q, hipStream_t sp)
{
    const int nw_max = q->nw_max, wpg = q->wpg;
    const long long tasks = (long long)c->n_streams * q->n_frames, per_wg = (long long)wpg * WAVE;
    if (q->ahead && c->free_armed[c->set]) HIPCHK(hipStreamWaitEvent(sp, c->ev_free[c->set], 0));      /* this set was last read by the synthesis of the call DEC_SETS back */
    /* The first parse-ahead behind an ordered call waits for all of it: that call's transform and synthesis read the first set of hand-over buffers, its
     * concealment kernel (on s) must not be overtaken by this call's (on s_plc, behind this parser) - both read-modify-write the concealment words
     * (DS_NBLOST, DS_CUM_ALPHA, DS_PLC_SEED, DS_PREV_BFI) - and with sizes from device memory its tail kernel writes the configuration this parser reads.
     * Every ordered call made today has completed when this wait is queued: the host-array calls return when they are done, and a call with sizes in
     * device memory (which returns before its work is done) leaves the host's copy of the configuration stale, so the fixed-size call that makes this
     * parse-ahead reads it back first (lc3_host.c dec_refresh), waiting for that call on the host.  The event states the order on the device instead of
     * leaving it to those host waits.  The other direction, an ordered call behind parse-ahead calls, waits on the device for the last of their
     * concealment kernels (ev_plc, dec_chain) - there a device-size call with sync = 0 does rely on it. */
    if (q->ahead && c->ord_pending) { HIPCHK(hipStreamWaitEvent(sp, c->ev_ord, 0)); c->ord_pending = 0; }
    /* How many parse waves a CU holds.  The kernel for frames of more than 128 bytes reads its frames from global memory and needs little LDS, so its 4 096
     * waves of 128 registers fill every SIMD, and the 64-wave concealment kernel and the transform of the call before wait for parse waves to retire; 24 KB of
     * padding per workgroup leave room beside them: d5 81.3 -> 88.7 Mframes/s (20 KB: 87.1, 28 KB: 77.1).  The kernel that stages its frames in LDS (d1) loses
     * with any padding (129 -> 117 at 16 KB): none there. */
    /* (the rule in bytes: the workgroup's LDS - tables, its waves' slices, padding - is a quarter of the CU's 160 KB, so that exactly four of them fit; that was 24 KB of padding
     * with the tables of the time) */
    const size_t quarter = (160u << 10) / 4, used = sizeof(ParseLds) + q->per_wave * wpg;
    const size_t pad = c->opt.dec_parse_pad_kb >= 0 ? (size_t)c->opt.dec_parse_pad_kb << 10 : (nw_max || used >= quarter ? 0 : quarter - used);
    /* `at`: where a stream's frames lie - the stride of the dense array, or (the _pk twins) the offsets of packed frames */
    auto parse = [&](auto kern, auto at) { LC3_LAUNCH(kern, dim3((unsigned)((tasks + per_wg - 1) / per_wg)), dim3(wpg * WAVE), q->per_wave * wpg + pad, sp, c->d_plan, c->d_chans, q->din, at, q->dbfi, q->dsizes, c->d_tab, q->n_frames, c->n_streams, nw_max, q->rec_w, q->ws_w, WS_ROW(c->N)); };
    if (q->offs_dev) parse(nw_max ? lc3_dec_parse_kernel_var_pk : lc3_dec_parse_kernel_g_var_pk, q->offs_dev);
    else parse(q->dsizes ? (nw_max ? lc3_dec_parse_kernel_var : lc3_dec_parse_kernel_g_var) : (nw_max ? lc3_dec_parse_kernel : lc3_dec_parse_kernel_g), q->in_stride);
    HIPCHK(hipGetLastError());
    return 0;
}
/* the stateful chain behind the parser (on sp).  Concealment bookkeeping: one channel-stream per lane; IMDCT: one channel-frame per wave; synthesis: one
 * channel-stream per wave (lc3_dec_kernels.inc).  With per-stream frame counts the _rag twins on the same grids as the dense call: a wave whose run of frames lies
 * past its stream's count returns at once, a stream without a present frame before touching its state */
static int dec_chain(lc3hip_dctx* c, const dec_call* q, hipStream_t sp)
{
    hipStream_t s = q->s;
    const int n_frames = q->n_frames; const int32_t* cnt = q->cnt;
    int* rec_w = q->rec_w; float* ws_w = q->ws_w; lc3d_dec_trace* dtr = q->dtr;
    /* The concealment bookkeeping needs its call's parser and the bookkeeping of the call before - NOT the transform or the synthesis of the call before.  On the caller's stream it
     * became runnable at the moment the NEXT call's parser did (both behind the previous synthesis; the parser waits for its set of hand-over buffers), lost the race for the SIMDs to
     * 4 096 parse waves of 128 registers, and took 0.9 ms for 0.05 ms of work - on the stream that bounds the call (timeline in profiles/experiments/r04_what_bounds.md, section 8).
     * On a stream of its own it runs the moment its parser ends, while the chip has room. */
    hipStream_t spl = s;
    if (q->ahead && c->opt.dec_plc_stream) {
        spl = c->s_plc;
        HIPCHK(hipEventRecord(c->ev_par[c->set], sp)); HIPCHK(hipStreamWaitEvent(spl, c->ev_par[c->set], 0));
    } else if (q->ahead) { HIPCHK(hipEventRecord(c->ev_par[c->set], sp)); HIPCHK(hipStreamWaitEvent(s, c->ev_par[c->set], 0)); }
    else if (c->s_plc) HIPCHK(hipStreamWaitEvent(s, c->ev_plc, 0));      /* an ordered call behind ahead calls: the bookkeeping is a chain (the event of the last one, if any: waiting on a fresh event is a no-op) */
    auto plc = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3((unsigned)((c->ncs + WAVE - 1) / WAVE)), dim3(WAVE), 0, spl, c->d_plan, c->d_chans, q->dsizes, c->d_tab, c->d_state, rec_w, n_frames, c->ncs, ragged...); };
    if (cnt) plc(lc3_dec_plc_kernel_rag, cnt); else plc(lc3_dec_plc_kernel);
    HIPCHK(hipGetLastError());
    if (spl != s) { HIPCHK(hipEventRecord(c->ev_plc, spl)); HIPCHK(hipStreamWaitEvent(s, c->ev_plc, 0)); }
    /* the IMDCT: four frames a wave at N = 480 in the standard layout (LC3PLUS_DEC_IMDCT4=0, or a traced call: the kernel below; a ragged call never carries a trace), else runs of IMDCT_FPW frames */
    auto imdct4 = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3((unsigned)((size_t)c->ncs * ((n_frames + 3) / 4))), dim3(WAVE), 0, s, c->d_plan, c->d_state, rec_w, ws_w, n_frames, c->ncs, c->d_ov, ragged...); };
    auto imdct = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3((unsigned)((size_t)c->ncs * ((n_frames + IMDCT_FPW - 1) / IMDCT_FPW))), dim3(WAVE), 0, s, c->d_plan, c->d_state, rec_w, ws_w, n_frames, c->ncs, c->d_ov, dtr, ragged...); };
    if (!c->big && c->opt.dec_imdct4 && !dtr && c->N == 480) { if (cnt) imdct4(lc3_dec_imdct4_kernel_rag, cnt); else imdct4(lc3_dec_imdct4_kernel); }
    else if (cnt) imdct(c->big ? lc3_dec_imdct_kernel_big_rag : lc3_dec_imdct_kernel_rag, cnt);
    else imdct(c->big ? lc3_dec_imdct_kernel_big : lc3_dec_imdct_kernel);
    /* the synthesis; placed PCM: the _plc twins */
    auto synth = [&](auto kern, auto... placed_ragged) { LC3_LAUNCH(kern, dim3(c->ncs), dim3(WAVE), 0, s, c->d_plan, c->d_state, rec_w, ws_w, c->d_ov, n_frames, q->dpcm, q->bps, c->ncs, q->dst, dtr, placed_ragged...); };
    if (cnt && c->plo) synth(c->big ? lc3_dec_synth_kernel_big_rag_plc : lc3_dec_synth_kernel_rag_plc, c->plo, c->plcap, cnt);
    else if (cnt) synth(c->big ? lc3_dec_synth_kernel_big_rag : lc3_dec_synth_kernel_rag, cnt);
    else if (c->plo) synth(c->big ? lc3_dec_synth_kernel_big_plc : lc3_dec_synth_kernel_plc, c->plo, c->plcap);
    else synth(c->big ? lc3_dec_synth_kernel_big : lc3_dec_synth_kernel);
    HIPCHK(hipGetLastError());
    return 0;
}
/* the tail of a call with sizes in device memory, the events later calls wait for, and what goes back to the host */
static int dec_tail(lc3hip_dctx* c, const dec_call* q)
{
    hipStream_t s = q->s;
    const int n_frames = q->n_frames;
    if (q->nb_dev) {                                                 /* behind the synthesis: the status bits and the stream's configuration for the next call */
        const long long n = (long long)c->n_streams * n_frames;
        auto tail = [&](auto kern, auto... ragged) { LC3_LAUNCH(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c->d_sizes, c->d_inval, c->d_tab, c->channels, c->n_streams, n_frames, c->d_chans, q->dst, ragged...); };
        /* the ragged tail also marks the invalid placements, among the present frames only */
        if (q->cnt) tail(lc3_dec_sizes_tail_kernel_rag, q->cnt, c->plo, c->plcap, c->N); else tail(lc3_dec_sizes_tail_kernel);
        HIPCHK(hipGetLastError());
        if (!q->cnt && placed_mark(c->plo, c->plcap, c->channels, c->N, n, q->dst, LC3D_DEC_ST_PCM_PLACE, s)) return 1;
    }
    if (q->ahead) { HIPCHK(hipEventRecord(c->ev_free[c->set], s)); c->free_armed[c->set] = 1; c->set = (c->set + 1) % DEC_SETS; }
    else if (c->s_par) { HIPCHK(hipEventRecord(c->ev_free[0], s)); c->free_armed[0] = 1; }      /* an ordered call reads the first set: a later parse-ahead into it waits for this one */
    if (!q->ahead && c->input_ready) {                               /* ... and the next parse-ahead waits for the whole call (dec_parse) */
        if (dec_side_streams(c)) return 1;
        HIPCHK(hipEventRecord(c->ev_ord, s)); c->ord_pending = 1;
    }
    c->last_stream = s;
    HIPCHK(hipEventRecord(c->ev1, s));
    if (!q->pcm_on_device) HIPCHK(hipMemcpyAsync(q->pcm, q->dpcm, q->pcm_bytes, hipMemcpyDeviceToHost, s));
    if (q->trace_host) HIPCHK(hipMemcpyAsync(q->trace_host, q->dtr, sizeof(lc3d_dec_trace) * (size_t)c->ncs * n_frames, hipMemcpyDeviceToHost, s));
    if (q->status_host) HIPCHK(hipMemcpyAsync(q->status_host, q->dst, (size_t)c->n_streams * n_frames, hipMemcpyDeviceToHost, s));
    if (q->sync || !q->pcm_on_device || !q->frames_on_device || q->trace_host || q->bfi_host || q->status_host) SYNC_TIMED(c, s);
    return 0;
}
static int dec_decode(lc3hip_dctx* c, dec_call* q, void* hip_stream)
{
    HIPCHK(hipSetDevice(c->device));
    if (c->plo && (!q->pcm_on_device || q->trace_host || (q->bps & LC3D_PCM_CHANNEL_MAJOR))) return 1;      /* placed PCM: device-pointer calls without traces (the host refuses the others) */
    q->cnt = c->counts ? c->d_cnt : nullptr;                       /* per-stream frame counts: the _rag kernels, every one behind the plan kernel that clamps them into d_cnt */
    if (q->cnt && !q->nb_dev) return 1;                             /* ... on the calls with sizes in device memory only (the host refuses the others) */
    hipStream_t s = q->s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (c->wk.calls && work_poison_all(&c->wk)) return 1;
    if (c->ss.done_armed) HIPCHK(hipStreamWaitEvent(s, c->ss.ev_done, 0));      /* behind the last stream-lifecycle call, whichever stream it was queued on */
    if (dec_stage(c, q) || dec_parse_lds(c, q)) return 1;
    hipStream_t sp = q->ahead ? c->s_par : s;
    HIPCHK(hipEventRecord(c->ev0, s));
    if (q->nb_dev && dec_plan(c, q)) return 1;
    return dec_parse(c, q, sp) || dec_chain(c, q, sp) || dec_tail(c, q);
}
extern "C" int lc3hip_dec_decode(void* ctx, const void* frames, int frames_on_device, int in_stride, const uint8_t* bfi_host, const uint16_t* sizes_host,
                                 int sizes_max_nbytes, int n_frames, void* pcm, int pcm_on_device, int bps, uint8_t* status_host, void* hip_stream, int sync,
                                 void* trace_host)
{
    dec_call q = {frames, frames_on_device, in_stride, bfi_host, sizes_host, sizes_max_nbytes, n_frames, pcm, pcm_on_device, bps, status_host, sync, trace_host};
    return dec_decode((lc3hip_dctx*)ctx, &q, hip_stream);
}
extern "C" int lc3hip_dec_decode_dsizes(void* ctx, const void* frames, int in_stride, const int32_t* num_bytes_dev, const uint8_t* bfi_dev, int n_frames,
                                        void* pcm, int bps, uint8_t* status_dev, void* hip_stream, int sync)
{
    dec_call q = {frames, 1, in_stride, nullptr, nullptr, 0, n_frames, pcm, 1, bps, nullptr, sync, nullptr, num_bytes_dev, bfi_dev, status_dev};
    return dec_decode((lc3hip_dctx*)ctx, &q, hip_stream);
}
extern "C" int lc3hip_dec_decode_packed(void* ctx, const void* frames, long long capacity, const long long* offsets_dev, const int32_t* num_bytes_dev, int max_bytes,
                                        const uint8_t* bfi_dev, int n_frames, void* pcm, int bps, uint8_t* status_dev, void* hip_stream, int sync)
{
    dec_call q = {frames, 1, max_bytes, nullptr, nullptr, 0, n_frames, pcm, 1, bps, nullptr, sync, nullptr, num_bytes_dev, bfi_dev, status_dev, offsets_dev, capacity};
    return dec_decode((lc3hip_dctx*)ctx, &q, hip_stream);
}
extern "C" int lc3hip_dec_stream_state(void* ctx, int mode, const int* streams, int n, const lc3d_dchan* cfg, void* blob, int blob_on_device, const uint32_t* hdr,
                                       uint8_t* status, void* hip_stream, int sync)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    /* behind the batch's last call: a parse-ahead call's concealment kernel (its stream's tail waits for it) and a device-size call's configuration tail included */
    if (ss_run(&c->ss, s, c->last_stream, mode, c->d_state, c->channels, streams, n, cfg, (int)sizeof(lc3d_dchan), c->d_chans, blob, blob_on_device, hdr, status, sync)) return 1;
    c->last_stream = s;
    /* the next parse-ahead reads the configuration and its concealment kernel the state this call writes: it waits for this call, as behind an ordered call */
    if (c->input_ready) { if (dec_side_streams(c)) return 1; HIPCHK(hipEventRecord(c->ev_ord, s)); c->ord_pending = 1; }
    return cfg ? dec_note_nbytes(c, cfg, 0, n * c->channels, streams) : 0;
}
extern "C" int lc3hip_dec_set_pcm_placement(void* ctx, const long long* offsets_dev, long long capacity)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    if (!c || capacity < 0) return 1;
    c->plo = offsets_dev; c->plcap = offsets_dev ? capacity : 0;
    return 0;
}
extern "C" int lc3hip_dec_set_frame_counts(void* ctx, const int32_t* counts_dev)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    if (!c) return 1;
    c->counts = counts_dev;
    return 0;
}
extern "C" int lc3hip_dec_set_input_ready(void* ctx, int ready)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    if (!c) return 1;
    /* 0 -> 1: an ordered call made before the promise may still be reading the first set of hand-over buffers, and it recorded no event a parse-ahead
     * could wait for (the side stream and its events exist from the first ahead call on): drain it once, as the encoder side does by clearing ahead_ok */
    if (ready && !c->input_ready && c->last_stream) { HIPCHK(hipSetDevice(c->device)); HIPCHK(hipStreamSynchronize(c->last_stream)); }
    c->input_ready = ready != 0;
    return 0;
}
extern "C" size_t lc3hip_dec_state_bytes(void* ctx) { lc3hip_dctx* c = (lc3hip_dctx*)ctx; return c ? sizeof(float) * (size_t)DST_WORDS * (size_t)c->ncs : 0; }
extern "C" int lc3hip_dec_get_state(void* ctx, void* host, size_t bytes)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    if (!c || !host || bytes != lc3hip_dec_state_bytes(ctx)) return 1;
    HIPCHK(hipSetDevice(c->device));
    if (c->last_stream) HIPCHK(hipStreamSynchronize(c->last_stream));
    HIPCHK(hipMemcpy(host, c->d_state, bytes, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int lc3hip_dec_set_state(void* ctx, const void* host, size_t bytes)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    if (!c || !host || bytes != lc3hip_dec_state_bytes(ctx)) return 1;
    HIPCHK(hipSetDevice(c->device));
    if (c->last_stream) HIPCHK(hipStreamSynchronize(c->last_stream));
    HIPCHK(hipMemcpy(c->d_state, host, bytes, hipMemcpyHostToDevice));
    return 0;
}
extern "C" float lc3hip_dec_last_ms(void* ctx) { return ctx ? ((lc3hip_dctx*)ctx)->last_ms : 0.0f; }
extern "C" int lc3hip_dec_probe_args(void* ctx, int* device, const lc3d_plan** plan_dev, const lc3d_dchan** tab_dev, int* tab_n, void** stream)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    if (!c || !c->d_plan || !c->d_tab) return 1;
    *device = c->device; *plan_dev = c->d_plan; *tab_dev = c->d_tab; *tab_n = c->tab_n; *stream = (void*)c->stream;
    return 0;
}
extern "C" int lc3hip_dec_destroy(void* ctx)
{
    lc3hip_dctx* c = (lc3hip_dctx*)ctx;
    if (!c) return 0;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    void* bufs[] = {c->d_plan, c->d_chans, c->d_state, c->d_in, c->d_pcm, c->d_bfi, c->d_trace, c->d_status, c->d_rec, c->d_ws, c->d_ov, c->d_tab, c->d_sizes, c->d_inval, c->d_cnt};
    for (int i = 0; i < DEC_SETS - 1; i++) { if (c->d_recx[i]) hipFree(c->d_recx[i]); if (c->d_wsx[i]) hipFree(c->d_wsx[i]); }
    if (c->s_par) { hipStreamDestroy(c->s_par); for (int i = 0; i < DEC_SETS; i++) { hipEventDestroy(c->ev_par[i]); hipEventDestroy(c->ev_free[i]); } hipStreamDestroy(c->s_plc); hipEventDestroy(c->ev_plc); hipEventDestroy(c->ev_ord); }
    for (void* p : bufs) if (p) hipFree(p);
    if (c->stream) hipStreamDestroy(c->stream);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    ss_free(&c->ss);
    free(c->h_nbytes);
    free(c);
    return 0;
}
