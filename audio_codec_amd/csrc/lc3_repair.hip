/* lc3_repair.hip -- the FEC repair library (liblc3plus_repair_hip.so): the gfx950 kernels of lc3_repair.inc and the host code that launches them, behind the C ABI
 * of lc3_repair_shim.h.  A sibling library (DESIGN.md "Sibling libraries"): lc3_packet.c loads it on the first repair call and hands it the batch's device and
 * stream.  It keeps no state but its launch counts and allocates nothing. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "lc3_repair_shim.h"

#define WAVE 64
#include "lc3_fec_xor.inc"
#include "lc3_repair.inc"

/* ---- host ---- */
#define SIB_NAME "lc3plus_repair"
#include "lc3_sibling.h"
static const sib_kernel k_table[] = {SIB_KERNEL(lc3_rep_fill_kernel), SIB_KERNEL(lc3_rep_first_kernel), SIB_KERNEL(lc3_rep_dist_kernel), SIB_KERNEL(lc3_rep_claim_kernel),
                                     SIB_KERNEL(lc3_rep_settle_kernel), SIB_KERNEL(lc3_rep_copy_kernel), SIB_KERNEL(lc3_rep_verdict_kernel),
                                     SIB_KERNEL(lc3_rep_rebuild_kernel), SIB_KERNEL(lc3_rep_report_kernel)};
extern "C" long long lc3rep_launch_count(const char* kernel) { return sib_launch_count(k_table, kernel); }

static inline int rep_pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && !(v & (v - 1)); }

extern "C" int lc3rep_repair_run(const lc3rep_call* q)
{
    if (!q) return 1;
    const lc3rep_io& io = q->io;
    if (io.n_streams < 1 || io.n_items < 0 || io.n_items >= LC3R_MAX_ITEMS || io.n_fec < 0 || io.n_fec >= LC3R_MAX_ITEMS || io.ring_capacity < 0) return 1;
    if (!rep_pow2_in(io.med_slots, LC3REP_MIN_MED, LC3REP_MAX_MED) || !rep_pow2_in(io.fec_slots, LC3REP_MIN_CELLS, LC3REP_MAX_CELLS)) return 1;
    if (io.med_stride < 16 || io.med_stride > LC3FEC_MAX_PKT || (io.med_stride & 15) || io.fec_stride < 16 || io.fec_stride > LC3FEC_MAX_PKT || (io.fec_stride & 15)) return 1;
    if (io.med_offset < 0 || (io.med_offset & 15) || io.passes < 1 || io.passes > LC3REP_MAX_PASSES) return 1;
    const long long nh = (long long)io.n_streams * io.med_slots, np = (long long)io.n_streams * io.fec_slots, items = io.n_items + io.n_fec;
    if (nh >= LC3FEC_MAX_PACKETS || np >= LC3FEC_MAX_PACKETS || io.med_offset > io.ring_capacity - nh * io.med_stride) return 1;
    if (!io.ring || !io.ssrc || !io.med_seq || !io.med_size || !io.fec_store || !io.cell_seq || !io.cell_size || !io.cell_status || !io.state || !io.rec_dg_offsets ||
        !io.rec_dg_sizes || !io.rec_seq || !q->work || ((uintptr_t)q->work & 7))
        return 1;
    if (io.n_items && (!io.dg_offsets || !io.dg_sizes || !io.stream || !io.seq)) return 1;
    if (io.n_fec && (!io.fec_stream || !io.fec_offsets || !io.fec_num_bytes || !io.fec_seq)) return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    const lc3rep_work w = lc3rep_work_of(q->work, io.n_streams, io.med_slots, io.fec_slots);
    const dim3 threads(LC3REP_THREADS);
    SIB_LAUNCH(lc3_rep_fill_kernel, dim3(sib_blocks_for(nh, LC3REP_THREADS, 1 << 14)), threads, 0, s, io, w);
    if (items) {
        const dim3 lanes((unsigned)((items + LC3REP_THREADS - 1) / LC3REP_THREADS));
        SIB_LAUNCH(lc3_rep_first_kernel, lanes, threads, 0, s, io, w);
        SIB_LAUNCH(lc3_rep_dist_kernel, lanes, threads, 0, s, io, w);
        SIB_LAUNCH(lc3_rep_claim_kernel, lanes, threads, 0, s, io, w);
    }
    SIB_LAUNCH(lc3_rep_settle_kernel, dim3((unsigned)((nh + np + LC3REP_THREADS - 1) / LC3REP_THREADS)), threads, 0, s, io, w);
    if (items) {
        const int per = LC3REP_THREADS / LC3REP_COPY_LANES;
        SIB_LAUNCH(lc3_rep_copy_kernel, dim3((unsigned)((items + per - 1) / per)), threads, 0, s, io, w);
    }
    const int per = LC3REP_THREADS / LC3FEC_REC_LANES;
    for (int p = 1; p <= io.passes; p++) {
        SIB_LAUNCH(lc3_rep_verdict_kernel, dim3((unsigned)((np + LC3REP_THREADS - 1) / LC3REP_THREADS)), threads, 0, s, io, w, p);
        SIB_LAUNCH(lc3_rep_rebuild_kernel, dim3((unsigned)((np + per - 1) / per)), threads, 0, s, io, w, p);
    }
    const long long rep = io.n_fec > io.n_streams ? io.n_fec : io.n_streams;
    SIB_LAUNCH(lc3_rep_report_kernel, dim3((unsigned)((rep + LC3REP_THREADS - 1) / LC3REP_THREADS)), threads, 0, s, io, w);
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}
