/* lc3_egress.hip -- the packet egress's library (liblc3plus_egress_hip.so): the gfx950 kernels of lc3_egress.inc and the host code that launches them, behind
 * the C ABI of lc3_egress_shim.h.  A sibling library (DESIGN.md "Sibling libraries"): lc3_packet.c loads it on the first egress call and hands it the batch's device
 * and stream count.  It keeps no state but its launch counts and allocates nothing. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "lc3_egress_shim.h"

#define WAVE 64
#include "lc3_egress.inc"

/* ---- host ---- */
#define SIB_NAME "lc3plus_egress"
#include "lc3_sibling.h"
static const sib_kernel k_table[] = {SIB_KERNEL(lc3_egress_classify_kernel), SIB_KERNEL(lc3_egress_sums_kernel), SIB_KERNEL(lc3_egress_base_kernel),
                                     SIB_KERNEL(lc3_egress_scatter_kernel), SIB_KERNEL(lc3_egress_route_kernel), SIB_KERNEL(lc3_egress_copy_kernel)};
extern "C" long long lc3egress_launch_count(const char* kernel) { return sib_launch_count(k_table, kernel); }

extern "C" int lc3egress_run(const lc3egress_call* q)
{
    if (!q || q->n_streams < 1 || q->n_frames <= 0 || q->n_routes <= 0 || (long long)q->n_routes * q->n_frames >= LC3E_MAX_CELLS) return 1;
    if (q->max_frame_bytes <= 0 || q->frames_capacity < 0 || q->wire_capacity < 0 || (q->seq_bits != 16 && q->seq_bits != 32)) return 1;
    if (q->order != LC3E_STREAM_MAJOR && q->order != LC3E_FRAME_MAJOR) return 1;
    if (q->header_room < 0 || q->align < 1 || q->align > LC3E_MAX_ALIGN || (q->align & (q->align - 1))) return 1;
    if (!q->wire && (q->header_room != 0 || q->align != 1)) return 1;
    if (!q->route_src && q->n_routes != q->n_streams) return 1;
    if (!q->frames || !q->offsets || !q->num_bytes || !q->seq_base || !q->list.route || !q->list.seq || !q->list.frame || !q->list.offset || !q->list.size ||
        !q->n_packets || !q->work || ((uintptr_t)q->work & 7))
        return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    const long long n_cells = (long long)q->n_routes * q->n_frames, n_tiles = lc3e_tiles(n_cells);
    const int wire_mode = q->wire != nullptr;
    int32_t* word = (int32_t*)q->work;
    long long* sums = (long long*)((char*)q->work + lc3e_work_sums(n_cells));
    lc3e_list L = q->list;                                            /* status: the caller's array, or the workspace's where the route kernel needs one */
    if (!L.status && q->stats) L.status = (uint8_t*)q->work + lc3e_work_status(n_cells);
    L.from = wire_mode ? (long long*)((char*)q->work + lc3e_work_from(n_cells)) : nullptr;
    SIB_LAUNCH(lc3_egress_classify_kernel, dim3((unsigned)((n_cells + LC3E_THREADS - 1) / LC3E_THREADS)), dim3(LC3E_THREADS), 0, s, n_cells, q->n_streams,
               q->n_routes, q->n_frames, q->order, q->route_src, q->counts, q->offsets, q->num_bytes, q->flags, q->max_frame_bytes, q->frames_capacity,
               q->skip_mask, word);
    SIB_LAUNCH(lc3_egress_sums_kernel, dim3((unsigned)n_tiles), dim3(LC3E_THREADS), 0, s, (const int32_t*)word, n_cells, wire_mode, q->header_room, q->align, sums);
    SIB_LAUNCH(lc3_egress_base_kernel, dim3(1), dim3(LC3E_THREADS), 0, s, sums, n_tiles, q->n_packets, q->wire_total);
    SIB_LAUNCH(lc3_egress_scatter_kernel, dim3((unsigned)n_tiles), dim3(LC3E_THREADS), 0, s, (const int32_t*)word, n_cells, (const long long*)sums, q->n_routes,
               q->n_frames, q->order, q->route_src, q->seq_base, q->seq_bits, q->offsets, wire_mode, q->header_room, q->align, q->wire_capacity, L);
    if (q->next_seq || q->stats) {
        SIB_LAUNCH(lc3_egress_route_kernel, dim3((unsigned)((q->n_routes + LC3E_THREADS / WAVE - 1) / (LC3E_THREADS / WAVE))), dim3(LC3E_THREADS), 0, s,
                   q->n_streams, q->n_routes, q->n_frames, q->route_src, q->counts, q->seq_base, q->seq_bits, (const uint8_t*)L.status, q->next_seq, q->stats);
    }
    if (wire_mode) {
        const int per = LC3E_THREADS / LC3E_COPY_LANES;              /* sized for every cell SENT: the workgroups behind *n_packets leave at once */
        SIB_LAUNCH(lc3_egress_copy_kernel, dim3((unsigned)((n_cells + per - 1) / per)), dim3(LC3E_THREADS), 0, s, (const uint8_t*)q->frames, q->frames_capacity,
                   (const long long*)q->n_packets, (const long long*)L.from, (const long long*)L.offset, (const int32_t*)L.size, q->header_room,
                   (uint8_t*)q->wire, q->wire_capacity);
    }
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}
