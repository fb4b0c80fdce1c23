/* lc3_rtp.hip -- the RTP framing's library (liblc3plus_rtp_hip.so): the gfx950 kernels of lc3_rtp.inc and the host code that launches them, behind the C ABI
 * of lc3_rtp_shim.h.  A sibling library (DESIGN.md "Sibling libraries"): lc3_packet.c loads it on the first RTP call and hands it the batch's device and stream
 * count.  It keeps no state but its launch counts and allocates nothing. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "lc3_rtp_shim.h"

#define WAVE 64
#include "lc3_rtp.inc"

/* ---- host ---- */
#define SIB_NAME "lc3plus_rtp"
#include "lc3_sibling.h"
static const sib_kernel k_table[] = {SIB_KERNEL(lc3_rtp_fill_kernel), SIB_KERNEL(lc3_rtp_parse_kernel), SIB_KERNEL(lc3_rtp_stamp_kernel), SIB_KERNEL(lc3_rtp_route_kernel)};
extern "C" long long lc3rtp_launch_count(const char* kernel) { return sib_launch_count(k_table, kernel); }

extern "C" int lc3rtp_parse_run(const lc3rtp_parse_call* q)
{
    if (!q || q->n_streams < 1 || q->n_items <= 0 || q->n_items >= LC3R_MAX_ITEMS || q->ring_capacity < 0 || q->n_ssrc <= 0) return 1;
    if (q->payload_room < 0 || q->payload_room > LC3R_MAX_PAYLOAD_ROOM) return 1;
    if (!q->ring || !q->dg_offsets || !q->dg_sizes || !q->ssrc_key || !q->ssrc_stream || !q->out.stream || !q->out.seq || !q->out.offsets || !q->out.num_bytes) return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    if (q->stats) {
        SIB_LAUNCH(lc3_rtp_fill_kernel, dim3(1), dim3(WAVE), 0, s, q->stats);
    }
    /* every workgroup stages the table it searches: one workgroup of 1 024 lanes per CU stages it once per CU and still fills half the CU's wave slots; the
     * grid stops there and walks the rest */
    const int lds_entries = q->n_ssrc <= LC3R_LDS_ENTRIES ? q->n_ssrc : 0;
    const long long want = (q->n_items + LC3R_PARSE_THREADS - 1) / LC3R_PARSE_THREADS, most = lds_entries ? 256 : 1024;
    SIB_LAUNCH(lc3_rtp_parse_kernel, dim3((unsigned)(want > most ? most : want)), dim3(LC3R_PARSE_THREADS), (size_t)lds_entries * 8, s,
               (const uint8_t*)q->ring, q->ring_capacity, q->dg_offsets, q->dg_sizes, q->n_items, q->ssrc_key, q->ssrc_stream, q->n_ssrc, lds_entries, q->n_streams,
               q->payload_type, q->payload_room, q->out, q->stats);
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int lc3rtp_stamp_run(const lc3rtp_stamp_call* q)
{
    if (!q || q->max_packets <= 0 || q->in.n_routes <= 0 || q->in.n_frames <= 0 || q->in.wire_capacity < 0 || q->in.payload_room < 0) return 1;
    if (q->in.header_room < LC3R_FIXED || q->in.header_room - LC3R_FIXED < q->in.payload_room) return 1;
    if (q->in.marker_mode != LC3R_MARKER_NEVER && q->in.marker_mode != LC3R_MARKER_AFTER_HOLE) return 1;
    if ((q->in.marker_mode == LC3R_MARKER_AFTER_HOLE || q->next_resume) && !q->in.cell_status) return 1;
    if (!q->n_packets || !q->in.route || !q->in.seq || !q->in.frame || !q->in.offset || !q->in.size || !q->in.ssrc || !q->in.ts_base || !q->in.payload_type || !q->wire)
        return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    /* sized for max_packets: the lanes behind *n_packets leave at once */
    SIB_LAUNCH(lc3_rtp_stamp_kernel, dim3(sib_blocks_for(q->max_packets, LC3R_THREADS, 1 << 16)), dim3(LC3R_THREADS), 0, s, q->in, q->max_packets, q->n_packets, (uint8_t*)q->wire,
               q->pkt_status);
    if (q->next_ts || q->next_resume) {
        SIB_LAUNCH(lc3_rtp_route_kernel, dim3(sib_blocks_for(q->in.n_routes, LC3R_THREADS, 1LL << 30)), dim3(LC3R_THREADS), 0, s, q->in, q->next_ts, q->next_resume);
    }
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}
