/* lc3_gcm.hip -- the Secure RTP AES-GCM library (liblc3plus_gcm_hip.so): the gfx950 kernels of lc3_gcm.inc and the host code that launches them, behind the C ABI
 * of lc3_gcm_shim.h.  A sibling library (DESIGN.md "Sibling libraries"): lc3_host.c loads it on the first GCM call and hands it the batch's device.  It keeps no
 * state but its launch counts, no key, and allocates nothing: all scratch lies in the caller's workspace. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "lc3_gcm_shim.h"

#define WAVE 64
#include "lc3_gcm.inc"

/* ---- host ---- */
#define SIB_NAME "lc3plus_gcm"
#include "lc3_sibling.h"
static const sib_kernel k_table[] = {SIB_KERNEL(lc3_gcm_protect_kernel), SIB_KERNEL(lc3_gcm_route_kernel), SIB_KERNEL(lc3_gcm_init_kernel),
                                     SIB_KERNEL(lc3_gcm_scan_kernel), SIB_KERNEL(lc3_gcm_auth_kernel), SIB_KERNEL(lc3_gcm_window_kernel),
                                     SIB_KERNEL(lc3_gcm_state_kernel)};
extern "C" long long lc3gcm_launch_count(const char* kernel) { return sib_launch_count(k_table, kernel); }

extern "C" int lc3gcm_protect_run(const lc3srtp_protect_call* q)
{
    if (!q || q->max_packets <= 0 || q->max_packets >= LC3S_MAX_ITEMS || !q->n_packets || q->in.n_routes <= 0 || q->in.tag_len != LC3G_TAG_BYTES) return 1;
    if (!q->in.route || !q->in.offset || !q->in.size || !q->in.status || !q->in.wire || !q->in.ctx || !q->in.roc || !q->in.seq_base || !q->in.dst) return 1;
    if (!q->out_offset || !q->out_size || !q->out_status || (q->next_roc && !q->in.next_seq)) return 1;
    if (q->in.dst_stride <= 0 || q->in.dst_stride > LC3S_MAX_STRIDE || q->in.dst_capacity < 0 || q->in.wire_capacity < 0) return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    const unsigned blocks = sib_blocks_for(q->max_packets, LC3S_THREADS, 1 << 16);
    SIB_LAUNCH(lc3_gcm_protect_kernel, dim3(blocks), dim3(LC3S_THREADS), 0, s, q->in, q->max_packets, q->n_packets, q->out_offset, q->out_size, q->out_status);
    if (q->next_roc) {
        SIB_LAUNCH(lc3_gcm_route_kernel, dim3(sib_blocks_for(q->in.n_routes, LC3S_THREADS, 1LL << 30)), dim3(LC3S_THREADS), 0, s, q->in, q->next_roc);
    }
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int lc3gcm_unprotect_run(const lc3srtp_unprotect_call* q)
{
    if (!q || q->n_items <= 0 || q->n_items >= LC3S_MAX_ITEMS || q->n_ssrc <= 0 || q->ring_capacity < 0 || q->tag_len != LC3G_TAG_BYTES) return 1;
    if (!q->ring || !q->dg_offsets || !q->dg_sizes || !q->ssrc_key || !q->ctx || !q->state_in || !q->state_out || !q->sizes_out || !q->workspace) return 1;
    if (q->workspace_bytes < lc3s_workspace_bytes(q->n_items, q->n_ssrc)) return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    /* the workspace's arrays (lc3_srtp_shim.h) */
    lc3g_work w;
    w.top1 = (unsigned long long*)(((uintptr_t)q->workspace + 15) & ~(uintptr_t)15);
    w.bits = w.top1 + q->n_ssrc;
    w.accepted = (long long*)(w.bits + q->n_ssrc);
    w.first = (int32_t*)(w.accepted + q->n_items);
    w.src = w.first + q->n_ssrc;
    const long long per_source = q->n_ssrc > LC3S_STATS_WORDS ? q->n_ssrc : LC3S_STATS_WORDS;
    SIB_LAUNCH(lc3_gcm_init_kernel, dim3(sib_blocks_for(per_source, LC3S_THREADS, 1LL << 30)), dim3(LC3S_THREADS), 0, s, w, q->n_ssrc, q->stats);
    const unsigned blocks = sib_blocks_for(q->n_items, LC3S_THREADS, 1 << 16);
    SIB_LAUNCH(lc3_gcm_scan_kernel, dim3(blocks), dim3(LC3S_THREADS), 0, s, *q, w);
    SIB_LAUNCH(lc3_gcm_auth_kernel, dim3(blocks), dim3(LC3S_THREADS), 0, s, *q, w);
    SIB_LAUNCH(lc3_gcm_window_kernel, dim3(blocks), dim3(LC3S_THREADS), 0, s, *q, w);
    SIB_LAUNCH(lc3_gcm_state_kernel, dim3(sib_blocks_for(q->n_ssrc, LC3S_THREADS, 1LL << 30)), dim3(LC3S_THREADS), 0, s, *q, w);
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}
