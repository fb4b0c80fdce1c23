/* lc3_srtp.hip -- the Secure RTP library (liblc3plus_srtp_hip.so): the gfx950 kernels of lc3_srtp.inc and the host code that launches them, behind the C ABI of
 * lc3_srtp_shim.h.  A seventh library beside liblc3plus_hip.so, liblc3plus_probe_hip.so, liblc3plus_ingest_hip.so, liblc3plus_egress_hip.so,
 * liblc3plus_rtp_hip.so and liblc3plus_rtcp_hip.so, so that the code objects of those six stay what they are; lc3_host.c loads it on the first call and hands it
 * the batch's device.  It keeps no state but its launch counts, no key, and allocates nothing: all scratch lies in the caller's workspace. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stddef.h>
#include <atomic>

#include "lc3_srtp_shim.h"

#define WAVE 64
#include "lc3_srtp.inc"

/* ---- host ---- */
enum { K_PROTECT = 0, K_ROUTE, K_INIT, K_SCAN, K_AUTH, K_WINDOW, K_STATE, K_COUNT };
static const char* const k_names[K_COUNT] = {"lc3_srtp_protect_kernel", "lc3_srtp_route_kernel", "lc3_srtp_init_kernel", "lc3_srtp_scan_kernel", "lc3_srtp_auth_kernel",
                                             "lc3_srtp_window_kernel", "lc3_srtp_state_kernel"};
static std::atomic<long long> k_launches[K_COUNT];
extern "C" long long lc3srtp_launch_count(const char* kernel)
{
    if (!kernel) return -1;
    for (int i = 0; i < K_COUNT; i++) if (!strcmp(kernel, k_names[i])) return k_launches[i].load(std::memory_order_relaxed);
    return -1;
}
#define QCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "lc3plus_srtp: %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

/* workgroups of LC3S_THREADS for n lanes of work, at most `most`: the kernels walk the rest grid-stride */
static unsigned blocks_for(long long n, long long most)
{
    const long long b = (n + LC3S_THREADS - 1) / LC3S_THREADS;
    return (unsigned)(b < 1 ? 1 : b > most ? most : b);
}

extern "C" int lc3srtp_protect_run(const lc3srtp_protect_call* q)
{
    if (!q || q->max_packets <= 0 || q->max_packets >= LC3S_MAX_ITEMS || !q->n_packets || q->in.n_routes <= 0 || (q->in.tag_len != 4 && q->in.tag_len != 10)) return 1;
    if (!q->in.route || !q->in.offset || !q->in.size || !q->in.status || !q->in.wire || !q->in.ctx || !q->in.roc || !q->in.seq_base || !q->in.dst) return 1;
    if (!q->out_offset || !q->out_size || !q->out_status || (q->next_roc && !q->in.next_seq)) return 1;
    if (q->in.dst_stride <= 0 || q->in.dst_stride > LC3S_MAX_STRIDE || q->in.dst_capacity < 0 || q->in.wire_capacity < 0) return 1;
    QCHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    const unsigned blocks = blocks_for(q->max_packets, 1 << 16);
    hipLaunchKernelGGL(lc3_srtp_protect_kernel, dim3(blocks), dim3(LC3S_THREADS), 0, s, q->in, q->max_packets, q->n_packets, q->out_offset, q->out_size, q->out_status);
    QCHK(hipGetLastError());
    k_launches[K_PROTECT]++;
    if (q->next_roc) {
        hipLaunchKernelGGL(lc3_srtp_route_kernel, dim3(blocks_for(q->in.n_routes, 1LL << 30)), dim3(LC3S_THREADS), 0, s, q->in, q->next_roc);
        QCHK(hipGetLastError());
        k_launches[K_ROUTE]++;
    }
    if (q->sync) QCHK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int lc3srtp_unprotect_run(const lc3srtp_unprotect_call* q)
{
    if (!q || q->n_items <= 0 || q->n_items >= LC3S_MAX_ITEMS || q->n_ssrc <= 0 || q->ring_capacity < 0 || (q->tag_len != 4 && q->tag_len != 10)) return 1;
    if (!q->ring || !q->dg_offsets || !q->dg_sizes || !q->ssrc_key || !q->ctx || !q->state_in || !q->state_out || !q->sizes_out || !q->workspace) return 1;
    if (q->workspace_bytes < lc3s_workspace_bytes(q->n_items, q->n_ssrc)) return 1;
    QCHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    /* the workspace's arrays (lc3_srtp_shim.h) */
    lc3s_work w;
    w.top1 = (unsigned long long*)(((uintptr_t)q->workspace + 15) & ~(uintptr_t)15);
    w.bits = w.top1 + q->n_ssrc;
    w.accepted = (long long*)(w.bits + q->n_ssrc);
    w.first = (int32_t*)(w.accepted + q->n_items);
    w.src = w.first + q->n_ssrc;
    const long long per_source = q->n_ssrc > LC3S_STATS_WORDS ? q->n_ssrc : LC3S_STATS_WORDS;
    hipLaunchKernelGGL(lc3_srtp_init_kernel, dim3(blocks_for(per_source, 1LL << 30)), dim3(LC3S_THREADS), 0, s, w, q->n_ssrc, q->stats);
    QCHK(hipGetLastError());
    k_launches[K_INIT]++;
    const unsigned blocks = blocks_for(q->n_items, 1 << 16);
    hipLaunchKernelGGL(lc3_srtp_scan_kernel, dim3(blocks), dim3(LC3S_THREADS), 0, s, *q, w);
    QCHK(hipGetLastError());
    k_launches[K_SCAN]++;
    hipLaunchKernelGGL(lc3_srtp_auth_kernel, dim3(blocks), dim3(LC3S_THREADS), 0, s, *q, w);
    QCHK(hipGetLastError());
    k_launches[K_AUTH]++;
    hipLaunchKernelGGL(lc3_srtp_window_kernel, dim3(blocks), dim3(LC3S_THREADS), 0, s, *q, w);
    QCHK(hipGetLastError());
    k_launches[K_WINDOW]++;
    hipLaunchKernelGGL(lc3_srtp_state_kernel, dim3(blocks_for(q->n_ssrc, 1LL << 30)), dim3(LC3S_THREADS), 0, s, *q, w);
    QCHK(hipGetLastError());
    k_launches[K_STATE]++;
    if (q->sync) QCHK(hipStreamSynchronize(s));
    return 0;
}
