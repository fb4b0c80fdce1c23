/* lc3_repair.inc -- the repair kernels of the generic FEC (included by lc3_repair.hip): this call's media and FEC items into the caller's per-stream stores, and
 * up to four passes of the stored FEC cells against the stored media, by the rule of include/lc3plus_batch.h "Generic FEC", REPAIR (lc3_repair_shim.h holds its
 * text, shared with lc3plus_plan_fec_repair on the host).  Every offset into the ring is 64 bits wide.
 *
 * fill resets the workspace's claims and zeroes the outputs; first, dist and claim run one lane per item (media and FEC in one launch): the lowest usable item of
 * a stream, its largest step ahead, the lowest item on each slot; settle runs one lane per slot and cell: expiry, the claim's outcome, the metadata; copy gives
 * LC3REP_COPY_LANES lanes to every item and moves the stored ones.  A pass is verdict, one lane per cell against the history as the pass found it, and rebuild, a
 * wave per cell that leaves at once unless its cell rebuilds.  report writes the FEC items' statuses and the streams' state.  No workgroup waits for another: the
 * kernel boundaries are the only ordering, integer atomicMin, atomicMax and atomicAdd the only traffic between workgroups. */

/* the claims and first become LC3FEC_NO_ENTRY, dist and the outputs 0, prog says that pass 1 runs */
extern "C" __global__ void __launch_bounds__(LC3REP_THREADS) lc3_rep_fill_kernel(lc3rep_io q, lc3rep_work w)
{
    const long long stride = (long long)gridDim.x * LC3REP_THREADS, i0 = (long long)blockIdx.x * LC3REP_THREADS + threadIdx.x;
    const long long n = q.n_streams, nh = n * q.med_slots, np = n * q.fec_slots;
    for (long long i = i0; i < 2 * n; i += stride) { w.first[i] = LC3FEC_NO_ENTRY; w.dist[i] = 0; }
    for (long long i = i0; i < nh; i += stride) { w.mclaim[i] = LC3FEC_NO_ENTRY; w.tclaim[i] = LC3FEC_NO_ENTRY; }
    for (long long i = i0; i < np; i += stride) { w.fclaim[i] = LC3FEC_NO_ENTRY; q.rec_dg_offsets[i] = 0; q.rec_dg_sizes[i] = 0; q.rec_seq[i] = 0; }
    if (i0 < LC3REP_PROG_WORDS) w.prog[i0] = i0 == 0;
    if (q.stats && i0 < LC3FEC_STATS_WORDS) q.stats[i0] = 0;
}

/* one item per lane, media first: step 0 the lowest usable item of its stream, 1 its step ahead of the base, 2 its claim on its slot */
template <int STEP>
__device__ __forceinline__ void lc3rep_item_lane(const lc3rep_io& q, const lc3rep_work& w)
{
    const long long e = (long long)blockIdx.x * LC3REP_THREADS + threadIdx.x;
    if (e >= q.n_items + q.n_fec) return;
    if (STEP == 0) lc3rep_first_step(&q, &w, e);
    else if (STEP == 1) lc3rep_dist_step(&q, &w, e);
    else lc3rep_claim_step(&q, &w, e);
}
extern "C" __global__ void __launch_bounds__(LC3REP_THREADS) lc3_rep_first_kernel(lc3rep_io q, lc3rep_work w) { lc3rep_item_lane<0>(q, w); }
extern "C" __global__ void __launch_bounds__(LC3REP_THREADS) lc3_rep_dist_kernel(lc3rep_io q, lc3rep_work w) { lc3rep_item_lane<1>(q, w); }
extern "C" __global__ void __launch_bounds__(LC3REP_THREADS) lc3_rep_claim_kernel(lc3rep_io q, lc3rep_work w) { lc3rep_item_lane<2>(q, w); }

/* one slot per lane, the media slots first, then the cells */
extern "C" __global__ void __launch_bounds__(LC3REP_THREADS) lc3_rep_settle_kernel(lc3rep_io q, lc3rep_work w)
{
    const long long i = (long long)blockIdx.x * LC3REP_THREADS + threadIdx.x, nh = (long long)q.n_streams * q.med_slots, np = (long long)q.n_streams * q.fec_slots;
    if (i < nh) lc3rep_settle_step(&q, &w, LC3REP_MED, i);
    else if (i < nh + np) lc3rep_settle_step(&q, &w, LC3REP_FEC, i - nh);
}

/* LC3REP_COPY_LANES lanes per item: its status, and a stored item's bytes into its slot or cell - exactly `size` of them, by the copy layout of the egress */
extern "C" __global__ void __launch_bounds__(LC3REP_THREADS) lc3_rep_copy_kernel(lc3rep_io q, lc3rep_work w)
{
    const int l = threadIdx.x & (LC3REP_COPY_LANES - 1);
    const long long e = ((long long)blockIdx.x * LC3REP_THREADS + threadIdx.x) / LC3REP_COPY_LANES;
    if (e >= q.n_items + q.n_fec) return;
    const lc3rep_item it = lc3rep_item_of(&q, e);
    long long slot = 0;
    const int st = lc3rep_place_step(&q, &w, &it, &slot);
    if (it.kind == LC3REP_MED && q.item_status && l == 0) q.item_status[e] = (uint8_t)st;
    if (st != LC3REP_STORED) return;
    const uintptr_t dst = it.kind == LC3REP_FEC ? (uintptr_t)q.fec_store + (uintptr_t)lc3rep_cell_at(&q, slot) : (uintptr_t)q.ring + (uintptr_t)lc3rep_slot_at(&q, slot);
    lc3fec_xor_store<LC3REP_COPY_LANES>(dst, it.size, 0, (const long long*)0, (const int32_t*)0, 0, (uintptr_t)q.ring + (uintptr_t)it.off, it.size, l);
}

/* the tallies of a workgroup go to stats with one atomic per word */
__device__ __forceinline__ void lc3rep_tally_out(const int* tally, int32_t* stats)
{
    __syncthreads();
    if (threadIdx.x < LC3REP_STATUSES && tally[threadIdx.x]) atomicAdd(stats + threadIdx.x, tally[threadIdx.x]);
}

/* One cell per lane: the verdict of pass p.  A pass behind one in which no cell rebuilt leaves at once */
extern "C" __global__ void __launch_bounds__(LC3REP_THREADS) lc3_rep_verdict_kernel(lc3rep_io q, lc3rep_work w, int p)
{
    __shared__ int tally[LC3REP_STATUSES];
    if (!w.prog[p - 1]) return;                                       /* the same in every lane of the grid */
    if (threadIdx.x < LC3REP_STATUSES) tally[threadIdx.x] = 0;
    __syncthreads();
    const long long c = (long long)blockIdx.x * LC3REP_THREADS + threadIdx.x;
    if (c < (long long)q.n_streams * q.fec_slots) {
        const int st = lc3rep_verdict_step(&q, &w, p, c);
        if (q.stats && st > 0 && st != LC3FEC_MISSING && lc3rep_carried(&w, c)) atomicAdd(&tally[st], 1);
    }
    if (q.stats) lc3rep_tally_out(tally, q.stats);
}

/* The rebuild kernel: a wave per cell, behind the verdict.  A cell that rebuilds nothing ends its wave at once.  Lane i folds the fields of the member at
 * position i of the mask and lists it; the present members, each cut to the protection length, and the level-0 payload are XORed into the media slot behind the
 * twelve header bytes that lane 0 writes with the slot's records */
extern "C" __global__ void __launch_bounds__(LC3REP_THREADS) lc3_rep_rebuild_kernel(lc3rep_io q, lc3rep_work w, int p)
{
    enum { PER = LC3REP_THREADS / LC3FEC_REC_LANES };
    __shared__ long long sh_at[PER][LC3FEC_MAX_BITS];
    __shared__ int32_t sh_len[PER][LC3FEC_MAX_BITS];
    __shared__ int tally[LC3REP_STATUSES];
    if (!w.prog[p]) return;                                           /* the same in every lane of the grid */
    if (threadIdx.x < LC3REP_STATUSES) tally[threadIdx.x] = 0;
    __syncthreads();
    const int l = threadIdx.x & (LC3FEC_REC_LANES - 1), slot = threadIdx.x / LC3FEC_REC_LANES;
    const long long c = (long long)blockIdx.x * PER + slot;
    lc3fec_item h;
    h.plen = 0; h.hl = 0; h.mask = 0; h.sn = 0; h.b0 = h.b1 = h.ts = h.len = 0;
    long long k = 0;
    uint32_t sn = 0;
    int st = -1;
    if (c < (long long)q.n_streams * q.fec_slots) {
        if (l == 0) st = lc3rep_rebuild_claim(&q, &w, c, &h, &k, &sn);
        st = __shfl(st, 0, LC3FEC_REC_LANES);                         /* lane 0 alone writes a TWIN's status */
    }
    int32_t rl = 0;
    if (st == LC3FEC_RECOVERED) {
        if (l != 0) { lc3rep_cell_header(&q, c, &h); sn = (uint32_t)w.verdict[c]; }
        k = (c / q.fec_slots) * q.med_slots + (sn & (uint32_t)(q.med_slots - 1));
        uint32_t hdr = 0, ts = 0, len = 0;
        if (l < LC3FEC_MAX_BITS) {
            long long at = 0;
            int32_t n = -1;
            const uint32_t mine = (h.sn + (uint32_t)l) & 0xFFFFu;
            if ((h.mask >> (LC3FEC_MAX_BITS - 1 - l) & 1) && mine != sn) {      /* every other member was present when the pass began */
                const long long m = (c / q.fec_slots) * q.med_slots + (mine & (uint32_t)(q.med_slots - 1));
                lc3rep_member_fields(&q, m, &hdr, &ts, &len);
                at = lc3rep_slot_at(&q, m) + LC3R_FIXED; n = (int32_t)len;
                if (n > (int32_t)h.plen) n = (int32_t)h.plen;
            }
            sh_at[slot][l] = at; sh_len[slot][l] = n;
        }
        for (int d = 1; d < LC3FEC_REC_LANES; d <<= 1) {
            hdr ^= __shfl_xor(hdr, d, LC3FEC_REC_LANES); ts ^= __shfl_xor(ts, d, LC3FEC_REC_LANES); len ^= __shfl_xor(len, d, LC3FEC_REC_LANES);
        }
        rl = (int32_t)(h.len ^ len);
        if (l == 0) lc3rep_rebuild_header(&q, c, &h, k, sn, hdr, ts, len);
    }
    __syncthreads();
    if (st == LC3FEC_RECOVERED)
        lc3fec_xor_store<LC3FEC_REC_LANES>((uintptr_t)q.ring + (uintptr_t)(lc3rep_slot_at(&q, k) + LC3R_FIXED), rl, (uintptr_t)q.ring, sh_at[slot], sh_len[slot],
                                           h.hl == LC3FEC_HEADER ? 16 : LC3FEC_MAX_BITS, (uintptr_t)q.fec_store + (uintptr_t)(lc3rep_cell_at(&q, c) + h.hl),
                                           (int32_t)h.plen, l);
    if (q.stats) {
        if (l == 0 && st >= 0 && lc3rep_carried(&w, c)) atomicAdd(&tally[st], 1);
        lc3rep_tally_out(tally, q.stats);
    }
}

/* one FEC item or stream per lane, behind the last pass: the items' statuses with their tallies, the streams' state */
extern "C" __global__ void __launch_bounds__(LC3REP_THREADS) lc3_rep_report_kernel(lc3rep_io q, lc3rep_work w)
{
    __shared__ int tally[LC3REP_STATUSES];
    if (threadIdx.x < LC3REP_STATUSES) tally[threadIdx.x] = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * LC3REP_THREADS + threadIdx.x;
    if (i < q.n_fec) {
        const int st = lc3rep_report_step(&q, &w, i);
        if (q.stats) atomicAdd(&tally[st], 1);
    }
    if (i < q.n_streams) lc3rep_state_step(&q, &w, (int)i);
    if (q.stats) lc3rep_tally_out(tally, q.stats);
}
