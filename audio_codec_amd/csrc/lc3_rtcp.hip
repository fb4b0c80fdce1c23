/* lc3_rtcp.hip -- the reception reports' library (liblc3plus_rtcp_hip.so): the gfx950 kernels of lc3_rtcp.inc and the host code that launches them, behind the
 * C ABI of lc3_rtcp_shim.h.  A sibling library (DESIGN.md "Sibling libraries"): lc3_packet.c loads it on the first call and hands it the batch's device.  It keeps no
 * state but its launch counts and allocates nothing: all scratch lies in the caller's workspace. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "lc3_rtcp_shim.h"

#define WAVE 64
#include "lc3_rtcp.inc"

/* ---- host ---- */
#define SIB_NAME "lc3plus_rtcp"
#include "lc3_sibling.h"
static const sib_kernel k_table[] = {SIB_KERNEL(lc3_rtcp_fill_kernel), SIB_KERNEL(lc3_rtcp_count_kernel), SIB_KERNEL(lc3_rtcp_scan_kernel),
                                     SIB_KERNEL(lc3_rtcp_scatter_kernel), SIB_KERNEL(lc3_rtcp_place_kernel), SIB_KERNEL(lc3_rtcp_walk_kernel)};
extern "C" long long lc3rtcp_launch_count(const char* kernel) { return sib_launch_count(k_table, kernel); }

extern "C" int lc3rtcp_stats_run(const lc3rtcp_stats_call* q)
{
    if (!q || q->n_streams <= 0 || q->n_items <= 0 || q->n_items >= LC3Q_MAX_ITEMS || (q->make_report != 0 && q->make_report != 1)) return 1;
    if (!q->stream || !q->seq || !q->timestamp || !q->arrival || !q->state_in || !q->state_out || !q->workspace) return 1;
    if (q->make_report && (!q->ssrc || !q->blocks)) return 1;
    if (q->workspace_bytes < lc3q_workspace_bytes(q->n_items, q->n_streams)) return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    /* the workspace's words (lc3_rtcp_shim.h) */
    const int most_big = (int)lc3q_most_big(q->n_items, q->n_streams);
    int32_t* off = (int32_t*)(((uintptr_t)q->workspace + 15) & ~(uintptr_t)15);
    int32_t* cur = off + q->n_streams + 1;
    int32_t* nbig = cur + q->n_streams;
    int32_t* big = nbig + 1;
    int32_t* idx = big + most_big;
    SIB_LAUNCH(lc3_rtcp_fill_kernel, dim3(sib_blocks_for((long long)q->n_streams + 1, LC3Q_THREADS, 1024)), dim3(LC3Q_THREADS), 0, s, cur, (long long)q->n_streams + 1);
    SIB_LAUNCH(lc3_rtcp_count_kernel, dim3(sib_blocks_for(q->n_items, LC3Q_THREADS, 1 << 16)), dim3(LC3Q_THREADS), 0, s, q->stream, q->n_items, q->n_streams, cur);
    SIB_LAUNCH(lc3_rtcp_scan_kernel, dim3(1), dim3(LC3Q_SCAN_THREADS), 0, s, off, cur, nbig, big, q->n_streams, most_big);
    SIB_LAUNCH(lc3_rtcp_scatter_kernel, dim3(sib_blocks_for(q->n_items, LC3Q_THREADS, 1 << 16)), dim3(LC3Q_THREADS), 0, s, q->stream, q->n_items, q->n_streams, off, cur, idx,
               q->ext_seq, q->item_status);
    if (most_big > 0) {                                              /* no stream can be long in a list of at most LC3Q_LDS_ITEMS items */
        SIB_LAUNCH(lc3_rtcp_place_kernel, dim3((unsigned)(most_big < 256 ? most_big : 256)), dim3(LC3Q_PLACE_THREADS), 0, s, q->stream, q->n_items, off, nbig, big,
                   most_big, idx);
    }
    SIB_LAUNCH(lc3_rtcp_walk_kernel, dim3((unsigned)(q->n_streams < (1 << 20) ? q->n_streams : 1 << 20)), dim3(LC3Q_WALK_THREADS), 0, s, *q, off, idx);
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}
