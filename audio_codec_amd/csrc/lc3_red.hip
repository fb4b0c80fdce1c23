/* lc3_red.hip -- the redundant-audio library (liblc3plus_red_hip.so): the gfx950 kernels of lc3_red.inc and the host code that launches them, behind the C ABI
 * of lc3_red_shim.h.  A sibling library (DESIGN.md "Sibling libraries"): lc3_packet.c loads it on the first RED call and hands it the batch's device and stream
 * count.  It keeps no state but its launch counts and allocates nothing. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "lc3_red_shim.h"

#define WAVE 64
#include "lc3_red.inc"

/* ---- host ---- */
#define SIB_NAME "lc3plus_red"
#include "lc3_sibling.h"
static const sib_kernel k_table[] = {SIB_KERNEL(lc3_red_size_kernel), SIB_KERNEL(lc3_red_sums_kernel), SIB_KERNEL(lc3_red_base_kernel), SIB_KERNEL(lc3_red_scatter_kernel),
                                     SIB_KERNEL(lc3_red_copy_kernel), SIB_KERNEL(lc3_red_tail_kernel), SIB_KERNEL(lc3_red_fill_kernel), SIB_KERNEL(lc3_red_unpack_kernel)};
extern "C" long long lc3red_launch_count(const char* kernel) { return sib_launch_count(k_table, kernel); }

extern "C" int lc3red_pack_run(const lc3red_pack_call* q)
{
    if (!q) return 1;
    const lc3red_pack_in& in = q->in;
    if (in.n_streams < 1 || in.n_frames <= 0 || in.n_routes <= 0 || in.max_frame_bytes <= 0 || in.frames_capacity < 0 || in.wire_capacity < 0) return 1;
    if (q->max_packets <= 0 || q->max_packets >= LC3RED_MAX_PACKETS || in.max_depth < 0 || in.max_depth > LC3RED_MAX_DEPTH || in.ts_step <= 0 || in.max_packet_bytes < 0) return 1;
    if (in.header_room < 0 || in.align < 1 || in.align > LC3E_MAX_ALIGN || (in.align & (in.align - 1))) return 1;
    if (!in.route_src && in.n_routes != in.n_streams) return 1;
    if (!in.tail_bytes != !in.tail_sizes || !q->tail_bytes_out != !q->tail_sizes_out) return 1;
    if (in.max_depth && (in.tail_sizes || q->tail_sizes_out) &&
        ((in.tail_stride & 15) || in.tail_stride < (in.max_frame_bytes < LC3RED_MAX_BLOCK ? in.max_frame_bytes : LC3RED_MAX_BLOCK)))
        return 1;
    if (!q->n_packets || !in.pkt_route || !in.pkt_frame || !in.frames || !in.offsets || !in.num_bytes || !in.block_pt || !q->wire || !q->red_offset || !q->red_size ||
        !q->work || ((uintptr_t)q->work & 7))
        return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    const long long n_tiles = lc3red_tiles(q->max_packets);
    int32_t* size = (int32_t*)q->work;
    long long* sums = (long long*)((char*)q->work + lc3red_work_sums(q->max_packets));
    uint8_t* mask = (uint8_t*)q->work + lc3red_work_mask(q->max_packets);
    /* every grid is sized for max_packets: the lanes behind *n_packets leave at once */
    SIB_LAUNCH(lc3_red_size_kernel, dim3((unsigned)((q->max_packets + LC3RED_THREADS - 1) / LC3RED_THREADS)), dim3(LC3RED_THREADS), 0, s, in, q->max_packets, q->n_packets,
               size, mask, q->route_stats);
    SIB_LAUNCH(lc3_red_sums_kernel, dim3((unsigned)n_tiles), dim3(LC3RED_THREADS), 0, s, (const int32_t*)size, q->max_packets, q->n_packets, in.align, sums);
    SIB_LAUNCH(lc3_red_base_kernel, dim3(1), dim3(LC3RED_THREADS), 0, s, sums, n_tiles, q->wire_total);
    SIB_LAUNCH(lc3_red_scatter_kernel, dim3((unsigned)n_tiles), dim3(LC3RED_THREADS), 0, s, (const int32_t*)size, (const uint8_t*)mask, q->max_packets, q->n_packets,
               (const long long*)sums, in.align, in.wire_capacity, q->red_offset, q->red_size, q->red_flags, q->red_blocks);
    const int per = LC3RED_THREADS / LC3RED_COPY_LANES;
    SIB_LAUNCH(lc3_red_copy_kernel, dim3((unsigned)((q->max_packets + per - 1) / per)), dim3(LC3RED_THREADS), 0, s, in, q->max_packets, q->n_packets, (const int32_t*)size,
               (const uint8_t*)mask, (const long long*)q->red_offset, (uint8_t*)q->wire, q->route_stats);
    if (q->tail_sizes_out && in.max_depth) {
        const long long entries = (long long)in.n_streams * in.max_depth;
        SIB_LAUNCH(lc3_red_tail_kernel, dim3((unsigned)((entries + per - 1) / per)), dim3(LC3RED_THREADS), 0, s, in, q->tail_bytes_out, q->tail_sizes_out);
    }
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int lc3red_unpack_run(const lc3red_unpack_call* q)
{
    if (!q) return 1;
    const lc3red_unpack_io& io = q->io;
    if (io.n_streams < 1 || q->n_items <= 0 || q->n_items >= LC3R_MAX_ITEMS || io.ring_capacity < 0 || io.max_red < 0 || io.max_red > LC3RED_MAX_DEPTH || io.ts_step <= 0) return 1;
    if (!io.stream || !io.seq || !io.offsets || !io.num_bytes || !io.ring || !io.out_stream || !io.out_seq || !io.out_offsets || !io.out_num_bytes) return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    if (q->stats) {
        SIB_LAUNCH(lc3_red_fill_kernel, dim3(1), dim3(WAVE), 0, s, q->stats);
    }
    SIB_LAUNCH(lc3_red_unpack_kernel, dim3(sib_blocks_for(q->n_items, LC3RED_THREADS, 1 << 12)), dim3(LC3RED_THREADS), 0, s, io, q->n_items, q->stats);
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}
