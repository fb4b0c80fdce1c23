/* lc3_fec.hip -- the generic-FEC library (liblc3plus_fec_hip.so): the gfx950 kernels of lc3_fec.inc and the host code that launches them, behind the C ABI of
 * lc3_fec_shim.h.  A sibling library (DESIGN.md "Sibling libraries"): lc3_packet.c loads it on the first FEC call and hands it the batch's device and stream.
 * It keeps no state but its launch counts and allocates nothing. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "lc3_fec_shim.h"

#define WAVE 64
#include "lc3_fec.inc"

/* ---- host ---- */
#define SIB_NAME "lc3plus_fec"
#include "lc3_sibling.h"
static const sib_kernel k_table[] = {SIB_KERNEL(lc3_fec_fill_kernel), SIB_KERNEL(lc3_fec_enc_scatter_kernel), SIB_KERNEL(lc3_fec_enc_sums_kernel),
                                     SIB_KERNEL(lc3_fec_enc_base_kernel), SIB_KERNEL(lc3_fec_enc_qbase_kernel), SIB_KERNEL(lc3_fec_enc_xor_kernel),
                                     SIB_KERNEL(lc3_fec_rec_scatter_kernel), SIB_KERNEL(lc3_fec_rec_verdict_kernel), SIB_KERNEL(lc3_fec_rec_bytes_kernel)};
extern "C" long long lc3fec_launch_count(const char* kernel) { return sib_launch_count(k_table, kernel); }

extern "C" int lc3fec_encode_run(const lc3fec_encode_call* q)
{
    if (!q) return 1;
    const lc3fec_enc_in& in = q->in;
    const lc3fec_enc_out& o = q->out;
    if (in.max_packets <= 0 || in.max_packets >= LC3FEC_MAX_PACKETS || in.n_routes <= 0 || in.n_frames <= 0 || (long long)in.n_routes * in.n_frames >= LC3E_MAX_CELLS) return 1;
    if (in.wire_capacity < 0 || in.payload_room < 0 || in.header_room < LC3R_FIXED + in.payload_room || in.max_fec_packets <= 0 || in.fec_capacity < 0) return 1;
    if (in.fec_stride <= 0 || in.fec_stride > LC3FEC_MAX_STRIDE || in.fec_header_room < LC3R_FIXED || in.fec_header_room > LC3FEC_MAX_PKT) return 1;
    if (!in.state_in != !in.acc_in || !o.state_out != !o.acc_out || !in.state_in != !o.state_out || in.carry != (o.state_out != NULL)) return 1;
    if (in.carry && (in.acc_stride <= 0 || (in.acc_stride & 15))) return 1;
    if (!in.n_packets || !in.pkt_route || !in.pkt_frame || !in.pkt_offset || !in.pkt_size || !in.wire || !in.seq_base || !in.group || !in.fec_seq_base || !o.n_fec ||
        !o.fec_route || !o.fec_seq || !o.fec_frame || !o.fec_offset || !o.fec_size || !o.fec_wire || !q->work || ((uintptr_t)q->work & 7))
        return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    const long long cells = (long long)in.n_routes * in.n_frames, n_tiles = lc3fec_tiles(in.n_routes);
    int32_t* map = (int32_t*)q->work;
    long long* sums = (long long*)((char*)q->work + lc3fec_work_sums(in.n_routes, in.n_frames));
    long long* qbase = (long long*)((char*)q->work + lc3fec_work_qbase(in.n_routes, in.n_frames));
    int32_t* fseq = (int32_t*)((char*)q->work + lc3fec_work_fseq(in.n_routes, in.n_frames));
    SIB_LAUNCH(lc3_fec_fill_kernel, dim3(sib_blocks_for(cells, LC3FEC_THREADS, 1 << 14)), dim3(LC3FEC_THREADS), 0, s, map, cells, (int32_t*)NULL, 0LL);
    /* sized for max_packets: the lanes behind *n_packets leave at once */
    SIB_LAUNCH(lc3_fec_enc_scatter_kernel, dim3((unsigned)((in.max_packets + LC3FEC_THREADS - 1) / LC3FEC_THREADS)), dim3(LC3FEC_THREADS), 0, s, in, map);
    SIB_LAUNCH(lc3_fec_enc_sums_kernel, dim3((unsigned)n_tiles), dim3(LC3FEC_THREADS), 0, s, in, sums);
    SIB_LAUNCH(lc3_fec_enc_base_kernel, dim3(1), dim3(LC3FEC_THREADS), 0, s, sums, n_tiles, o.n_fec);
    SIB_LAUNCH(lc3_fec_enc_qbase_kernel, dim3((unsigned)n_tiles), dim3(LC3FEC_THREADS), 0, s, in, (const long long*)sums, qbase, fseq, o.next_fec_seq, o.route_stats_out);
    const int per = LC3FEC_THREADS / LC3FEC_ENC_LANES;
    const long long slots = (long long)in.n_routes * ((long long)in.n_frames + 1);
    SIB_LAUNCH(lc3_fec_enc_xor_kernel, dim3((unsigned)((slots + per - 1) / per)), dim3(LC3FEC_THREADS), 0, s, in, o, (const int32_t*)map, (const long long*)qbase, (const int32_t*)fseq);
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int lc3fec_recover_run(const lc3fec_recover_call* q)
{
    if (!q) return 1;
    const lc3fec_rec_io& io = q->io;
    if (io.n_streams < 1 || io.n_items <= 0 || io.n_items >= LC3R_MAX_ITEMS || io.n_fec <= 0 || io.n_fec >= LC3R_MAX_ITEMS || io.ring_capacity < 0) return 1;
    if (io.window < 64 || io.window > 65536 || (io.window & (io.window - 1)) || io.rec_offset < 0 || io.rec_stride < LC3R_FIXED || io.rec_stride > LC3FEC_MAX_STRIDE) return 1;
    if (!io.ring || !io.dg_offsets || !io.dg_sizes || !io.stream || !io.seq || !io.fec_stream || !io.fec_offsets || !io.fec_num_bytes || !io.ssrc || !io.rec_dg_offsets ||
        !io.rec_dg_sizes || !io.rec_seq || !q->work || ((uintptr_t)q->work & 7))
        return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    int32_t* table = (int32_t*)q->work;
    const long long words = (long long)io.n_streams * io.window;
    SIB_LAUNCH(lc3_fec_fill_kernel, dim3(sib_blocks_for(words, LC3FEC_THREADS, 1 << 14)), dim3(LC3FEC_THREADS), 0, s, table, words, q->stats, (long long)LC3FEC_STATS_WORDS);
    SIB_LAUNCH(lc3_fec_rec_scatter_kernel, dim3((unsigned)((io.n_items + LC3FEC_THREADS - 1) / LC3FEC_THREADS)), dim3(LC3FEC_THREADS), 0, s, io, table);
    SIB_LAUNCH(lc3_fec_rec_verdict_kernel, dim3(sib_blocks_for(io.n_fec, LC3FEC_THREADS, 1 << 12)), dim3(LC3FEC_THREADS), 0, s, io, (const int32_t*)table, q->stats);
    const int per = LC3FEC_THREADS / LC3FEC_REC_LANES;
    SIB_LAUNCH(lc3_fec_rec_bytes_kernel, dim3((unsigned)((io.n_fec + per - 1) / per)), dim3(LC3FEC_THREADS), 0, s, io, (const int32_t*)table);
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}
