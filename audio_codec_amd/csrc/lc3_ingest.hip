/* lc3_ingest.hip -- the packet ingest's library (liblc3plus_ingest_hip.so): the gfx950 kernels of lc3_ingest.inc and the host code that launches them, behind the
 * C ABI of lc3_ingest_shim.h.  A sibling library (DESIGN.md "Sibling libraries"): lc3_packet.c loads it on the first lc3plus_dec_batch_ingest call and hands it the
 * batch's device, stream count and channel count.  It keeps no state but its launch counts and allocates nothing. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "lc3_ingest_shim.h"

#define WAVE 64
#include "lc3_ingest.inc"

/* ---- host ---- */
#define SIB_NAME "lc3plus_ingest"
#include "lc3_sibling.h"
static const sib_kernel k_table[] = {SIB_KERNEL(lc3_ingest_fill_kernel), SIB_KERNEL(lc3_ingest_item_kernel), SIB_KERNEL(lc3_ingest_stream_kernel),
                                     SIB_KERNEL(lc3_ingest_status_kernel)};
extern "C" long long lc3ingest_launch_count(const char* kernel) { return sib_launch_count(k_table, kernel); }

extern "C" int lc3ingest_run(const lc3ingest_call* q)
{
    if (!q || q->n_items <= 0 || q->n_items >= LC3I_MAX_ITEMS || q->n_streams < 1 || q->channels < 1 || q->n_frames <= 0 || (q->seq_bits != 16 && q->seq_bits != 32))
        return 1;
    if (!q->stream || !q->seq || !q->offsets || !q->num_bytes || !q->base || !q->out_offsets || !q->out_num_bytes || !q->cell_item || !q->counts) return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    const long long n_cells = (long long)q->n_streams * q->n_frames;
    const unsigned item_blocks = sib_blocks_for(q->n_items, 256, 1 << 14);
    SIB_LAUNCH(lc3_ingest_fill_kernel, dim3(sib_blocks_for(n_cells, 256, 1 << 14)), dim3(256), 0, s, (uint32_t*)q->cell_item, n_cells, q->stats,
               (long long)q->n_streams * LC3I_STATS_WORDS);
    SIB_LAUNCH(lc3_ingest_item_kernel, dim3(item_blocks), dim3(256), 0, s, q->stream, q->seq, q->num_bytes, q->info, q->base, q->n_items, q->n_streams,
               q->channels, q->seq_bits, q->n_frames, (uint32_t*)q->cell_item, q->stats);
    SIB_LAUNCH(lc3_ingest_stream_kernel, dim3((unsigned)((q->n_streams + 3) / 4)), dim3(4 * WAVE), 0, s, q->offsets, q->num_bytes, q->base, q->floor,
               q->n_streams, q->seq_bits, q->n_frames, q->out_offsets, q->out_num_bytes, q->cell_item, q->counts, q->next_base, q->stats);
    if (q->item_status) {
        SIB_LAUNCH(lc3_ingest_status_kernel, dim3(item_blocks), dim3(256), 0, s, q->stream, q->seq, q->num_bytes, q->info, q->base, q->n_items, q->n_streams,
                   q->channels, q->seq_bits, q->n_frames, q->cell_item, q->item_status);
    }
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}
