/* lc3_fec.inc -- the generic-FEC kernels (included by lc3_fec.hip): the stamped packet list and its wire buffer -> RFC 5109 parity packets in a wire buffer of
 * their own, and received media and FEC items -> recovered RTP packets in the ring, by the rules of include/lc3plus_batch.h "Generic FEC" (lc3_fec_shim.h holds
 * their text, shared with lc3plus_plan_fec_encode and lc3plus_plan_fec_recover on the host).  Every offset into the wire buffers and the ring is 64 bits wide.
 *
 * The encoder: fill and scatter write the cell-to-entry map into the caller's workspace (atomicMin: the lowest entry wins); sums reduces the closed-group counts
 * of each tile of LC3FEC_TILE routes, one lane per route doing the group arithmetic; base, one workgroup, turns the tiles' sums into their bases and writes
 * *n_fec; qbase scans each tile once more and writes every route's first entry, a copy of its fec_seq_base and its next sequence number; xor, the only kernel that touches payload bytes, gives
 * LC3FEC_ENC_LANES lanes to every group a route touches.  The recovery: fill and scatter write the lookup table; verdict runs one lane per FEC item; bytes gives
 * a wave to every item and leaves at once unless the item recovers.  No workgroup waits for another: the kernel boundaries are the only ordering. */

/* exclusive scan of v over the workgroup by wave-level scans and one exchange of the waves' sums; the workgroup's sum in *all.  sh: LC3FEC_THREADS / WAVE entries */
__device__ __forceinline__ void lc3fec_block_scan(long long* v, long long* all, long long* sh)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, waves = blockDim.x / WAVE;
    long long b = *v;
    for (int d = 1; d < WAVE; d <<= 1) {
        const long long ob = __shfl_up(b, d, WAVE);
        if (lane >= d) b += ob;
    }
    __syncthreads();                                                  /* the previous use of sh is over */
    if (lane == WAVE - 1) sh[wave] = b;
    __syncthreads();
    long long pb = 0, tb = 0;
    for (int w = 0; w < waves; w++) { const long long wb = sh[w]; if (w < wave) pb += wb; tb += wb; }
    *v = pb + b - *v;
    *all = tb;
}

/* n words of a map or table become LC3FEC_NO_ENTRY; the first lanes also zero n_zero words at `zero` (stats) */
extern "C" __global__ void __launch_bounds__(LC3FEC_THREADS) lc3_fec_fill_kernel(int32_t* __restrict__ map, long long n, int32_t* __restrict__ zero, long long n_zero)
{
    const long long stride = (long long)gridDim.x * LC3FEC_THREADS, i0 = (long long)blockIdx.x * LC3FEC_THREADS + threadIdx.x;
    for (long long i = i0; i < n; i += stride) map[i] = LC3FEC_NO_ENTRY;
    if (zero)
        for (long long i = i0; i < n_zero; i += stride) zero[i] = 0;
}

/* one list entry per lane: a member's cell learns the entry, the lowest of those that name it */
extern "C" __global__ void __launch_bounds__(LC3FEC_THREADS) lc3_fec_enc_scatter_kernel(lc3fec_enc_in q, int32_t* __restrict__ map)
{
    const long long p = (long long)blockIdx.x * LC3FEC_THREADS + threadIdx.x;
    if (p >= lc3fec_count(q.n_packets, q.max_packets)) return;
    const long long cell = lc3fec_entry_cell(&q, p);
    if (cell >= 0) atomicMin(map + cell, (int32_t)p);
}

/* one tile per workgroup: sums[tile] = the groups its routes close */
extern "C" __global__ void __launch_bounds__(LC3FEC_THREADS) lc3_fec_enc_sums_kernel(lc3fec_enc_in q, long long* __restrict__ sums)
{
    __shared__ long long sh[LC3FEC_THREADS / WAVE];
    const long long r0 = (long long)blockIdx.x * LC3FEC_TILE + (long long)threadIdx.x * LC3FEC_ITEMS;
    long long n = 0, all;
    for (int k = 0; k < LC3FEC_ITEMS; k++)
        if (r0 + k < q.n_routes) n += lc3fec_route_plan(&q, (int)(r0 + k)).nclosed;
    lc3fec_block_scan(&n, &all, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

/* one workgroup: the tiles' sums -> the tiles' bases, in place, and the call's *n_fec */
extern "C" __global__ void __launch_bounds__(LC3FEC_THREADS) lc3_fec_enc_base_kernel(long long* __restrict__ sums, long long n_tiles, long long* __restrict__ n_fec)
{
    __shared__ long long sh[LC3FEC_THREADS / WAVE];
    long long run = 0;
    for (long long b0 = 0; b0 < n_tiles; b0 += LC3FEC_THREADS) {
        const long long b = b0 + threadIdx.x;
        long long n = b < n_tiles ? sums[b] : 0, all;
        lc3fec_block_scan(&n, &all, sh);
        if (b < n_tiles) sums[b] = run + n;
        run += all;
    }
    if (threadIdx.x == 0) *n_fec = run;
}

/* one tile per workgroup, behind the base kernel: every route's first entry, its next FEC sequence number, and its stats zeroed for the xor kernel */
extern "C" __global__ void __launch_bounds__(LC3FEC_THREADS) lc3_fec_enc_qbase_kernel(lc3fec_enc_in q, const long long* __restrict__ base, long long* __restrict__ qbase,
                                                                                      int32_t* __restrict__ fseq, int32_t* next_fec_seq,
                                                                                      int32_t* __restrict__ route_stats_out)
{
    __shared__ long long sh[LC3FEC_THREADS / WAVE];
    const long long r0 = (long long)blockIdx.x * LC3FEC_TILE + (long long)threadIdx.x * LC3FEC_ITEMS;
    int w[LC3FEC_ITEMS];
    long long n = 0, all;
#pragma unroll
    for (int k = 0; k < LC3FEC_ITEMS; k++) {
        w[k] = r0 + k < q.n_routes ? lc3fec_route_plan(&q, (int)(r0 + k)).nclosed : 0;
        n += w[k];
    }
    lc3fec_block_scan(&n, &all, sh);
    long long run = base[blockIdx.x] + n;
#pragma unroll
    for (int k = 0; k < LC3FEC_ITEMS; k++) {
        const long long r = r0 + k;
        if (r >= q.n_routes) break;
        qbase[r] = run;
        const int32_t seq0 = q.fec_seq_base[r];                      /* read before next_fec_seq, which may be the same word, is written */
        fseq[r] = seq0;
        if (next_fec_seq) next_fec_seq[r] = (int32_t)((uint32_t)seq0 + (uint32_t)w[k]);
        if (route_stats_out)
            for (int j = 0; j < LC3FEC_RS_WORDS; j++) route_stats_out[r * LC3FEC_RS_WORDS + j] = 0;
        run += w[k];
    }
}

#include "lc3_fec_xor.inc"

/* The xor kernel: LC3FEC_ENC_LANES lanes per slot (r, g), g in 0 ... n_frames.  Slot g < ng is group g of the route's plan: its lanes list the members of its
 * positions in LDS, lane 0 folds the header fields and writes the record and the fourteen header bytes (a closed group) or the state (an open one), and all
 * lanes XOR the payload - behind the carried accumulator - into the FEC packet or into acc_out.  The last slot serves a route that leaves no open group: its
 * state and accumulator are handed through (c = 0) or zeroed.  The workgroup then adds its packets to their routes' stats, neighbours of one route summed in LDS
 * first (the RED copy kernel's way), which the qbase kernel has zeroed. */
extern "C" __global__ void __launch_bounds__(LC3FEC_THREADS) lc3_fec_enc_xor_kernel(lc3fec_enc_in q, lc3fec_enc_out o, const int32_t* __restrict__ map,
                                                                                    const long long* __restrict__ qbase, const int32_t* __restrict__ fseq)
{
    enum { PER = LC3FEC_THREADS / LC3FEC_ENC_LANES };
    __shared__ long long sh_at[PER][LC3FEC_MAX_GROUP];
    __shared__ int32_t sh_len[PER][LC3FEC_MAX_GROUP];
    __shared__ int32_t sh_plen[PER], sh_mode[PER], sh_r[PER], sh_pk[PER], sh_md[PER], sh_by[PER];
    __shared__ long long sh_dst[PER];
    const int l = threadIdx.x & (LC3FEC_ENC_LANES - 1), slot = threadIdx.x / LC3FEC_ENC_LANES;
    const long long e = (long long)blockIdx.x * PER + slot, per_route = (long long)q.n_frames + 1;
    const int live = e < (long long)q.n_routes * per_route;
    const int r = live ? (int)(e / per_route) : 0, g = live ? (int)(e - (long long)r * per_route) : 0;
    lc3fec_plan P;
    lc3fec_group G;
    P.c = P.F = P.K = P.k = P.a = P.ng = P.nclosed = P.open = 0;
    G.t0 = G.t1 = G.K = G.F0 = G.closes = 0;
    int is_group = 0;
    if (live) {
        P = lc3fec_route_plan(&q, r);
        is_group = g < P.ng;
        if (is_group) {
            G = lc3fec_group_of(&P, g);
            for (int i = l; i < G.t1 - G.t0; i += LC3FEC_ENC_LANES) {
                long long at = 0;
                int32_t len = -1;
                if (!lc3fec_member(&q, map, r, G.t0 + i, &at, &len)) len = -1;
                sh_at[slot][i] = at; sh_len[slot][i] = len;
            }
        }
    }
    __syncthreads();
    /* lane 0: mode 0 nothing to XOR, 1 into the FEC packet, 2 into acc_out; plen and dst for the other lanes; the stats of this slot */
    if (l == 0) {
        int mode = 0, plen = 0, pk = 0, md = 0, by = 0, rr = -1;
        long long dst = 0;
        if (is_group) {
            const lc3fec_fold f = lc3fec_fold_group(&q, r, &G, sh_at[slot], sh_len[slot]);
            plen = f.plen;
            if (G.closes) {
                const long long en = qbase[r] + g;
                int32_t size = 0;
                rr = r;
                if (lc3fec_emit(&q, &o, r, g, &G, &f, en, fseq[r], &size)) {
                    uint32_t w[4];
                    dst = en * q.fec_stride + q.fec_header_room;
                    lc3fec_header(&f, w);
                    lc3fec_header_out(o.fec_wire + dst, w);
                    dst += LC3FEC_HEADER; mode = 1; pk = 1; md = __popc(f.mask); by = plen;
                }
            } else if (q.carry) {
                if (lc3fec_state_out(&q, o.state_out + (size_t)r * LC3FEC_STATE_WORDS, &G, &f)) mode = 2; else { mode = 3; plen = 0; }
                dst = (long long)r * q.acc_stride;
            }
        } else if (live && g == q.n_frames && q.carry && !P.open) {
            int32_t* st = o.state_out + (size_t)r * LC3FEC_STATE_WORDS;
            const int through = P.c == 0 && q.state_in;
            for (int j = 0; j < LC3FEC_STATE_WORDS; j++) st[j] = through ? q.state_in[(size_t)r * LC3FEC_STATE_WORDS + j] : 0;
            mode = through ? 4 : 3;
            dst = (long long)r * q.acc_stride;
        }
        sh_plen[slot] = plen; sh_mode[slot] = mode; sh_dst[slot] = dst; sh_r[slot] = rr; sh_pk[slot] = pk; sh_md[slot] = md; sh_by[slot] = by;
    }
    __syncthreads();
    {
        const int mode = sh_mode[slot], plen = sh_plen[slot], cnt = is_group ? G.t1 - G.t0 : 0;
        const long long dst = sh_dst[slot];
        /* the carried accumulator counts up to the length the state names */
        int32_t xlen = 0;
        if (is_group && G.F0 > 0 && (mode == 1 || mode == 2)) {
            xlen = q.state_in[(size_t)r * LC3FEC_STATE_WORDS + LC3FEC_S_MAX];
            xlen = xlen < 0 || xlen > q.acc_stride || xlen > plen ? 0 : xlen;
        }
        const uintptr_t xsrc = (uintptr_t)q.acc_in + (uintptr_t)r * (uintptr_t)q.acc_stride;
        if (mode == 1) lc3fec_xor_store<LC3FEC_ENC_LANES>((uintptr_t)o.fec_wire + (uintptr_t)dst, plen, (uintptr_t)q.wire, sh_at[slot], sh_len[slot], cnt, xsrc, xlen, l);
        else if (mode == 2) lc3fec_xor_store<LC3FEC_ENC_LANES>((uintptr_t)o.acc_out + (uintptr_t)dst, q.acc_stride, (uintptr_t)q.wire, sh_at[slot], sh_len[slot], cnt, xsrc, xlen, l);
        else if (mode == 3) lc3fec_xor_store<LC3FEC_ENC_LANES>((uintptr_t)o.acc_out + (uintptr_t)dst, q.acc_stride, 0, sh_at[slot], sh_len[slot], 0, 0, 0, l);
        else if (mode == 4) lc3fec_xor_store<LC3FEC_ENC_LANES>((uintptr_t)o.acc_out + (uintptr_t)dst, q.acc_stride, 0, sh_at[slot], sh_len[slot], 0, xsrc, q.acc_stride, l);
    }
    if (!o.route_stats_out) return;                                   /* the same in every lane of the grid */
    if (threadIdx.x < PER && sh_r[threadIdx.x] >= 0 && (threadIdx.x == 0 || sh_r[threadIdx.x - 1] != sh_r[threadIdx.x])) {
        const int r0 = sh_r[threadIdx.x];
        int groups = 0, packets = 0, media = 0, bytes = 0;
        for (int i = threadIdx.x; i < PER && sh_r[i] == r0; i++) { groups++; packets += sh_pk[i]; media += sh_md[i]; bytes += sh_by[i]; }
        int32_t* st = o.route_stats_out + (size_t)r0 * LC3FEC_RS_WORDS;
        atomicAdd(st + LC3FEC_RS_GROUPS, groups);
        if (packets) { atomicAdd(st + LC3FEC_RS_PACKETS, packets); atomicAdd(st + LC3FEC_RS_MEDIA, media); atomicAdd(st + LC3FEC_RS_BYTES, bytes); }
    }
}

/* one media item per lane: a usable item enters the table at its residue, the lowest item index of those that share it */
extern "C" __global__ void __launch_bounds__(LC3FEC_THREADS) lc3_fec_rec_scatter_kernel(lc3fec_rec_io q, int32_t* __restrict__ table)
{
    const long long i = (long long)blockIdx.x * LC3FEC_THREADS + threadIdx.x;
    if (i >= q.n_items) return;
    const int s = q.stream[i];
    if (s < 0 || s >= q.n_streams) return;
    atomicMin(table + (size_t)s * q.window + ((uint32_t)q.seq[i] & (uint32_t)(q.window - 1)), (int32_t)i);
}

/* One FEC item per lane, grid-stride: the verdict.  stats: the lanes tally in LDS, the workgroup adds its sums with one vector atomic per word at its end */
extern "C" __global__ void __launch_bounds__(LC3FEC_THREADS) lc3_fec_rec_verdict_kernel(lc3fec_rec_io q, const int32_t* __restrict__ table, int32_t* __restrict__ stats)
{
    __shared__ int tally[LC3FEC_STATUSES];
    if (threadIdx.x < LC3FEC_STATUSES) tally[threadIdx.x] = 0;
    __syncthreads();
    const long long stride = (long long)gridDim.x * LC3FEC_THREADS;
    for (long long f = (long long)blockIdx.x * LC3FEC_THREADS + threadIdx.x; f < q.n_fec; f += stride) {
        const int st = lc3fec_verdict(&q, table, f);
        if (stats) atomicAdd(&tally[st], 1);
    }
    if (stats) {
        __syncthreads();
        if (threadIdx.x < LC3FEC_STATUSES && tally[threadIdx.x]) atomicAdd(stats + threadIdx.x, tally[threadIdx.x]);
    }
}

/* The byte kernel: a wave per FEC item, behind the verdict.  An item that did not recover (rec_dg_sizes 0) ends its wave at once.  Lane i looks position i of the
 * mask up; the present packets, each cut to the protection length, and the level-0 payload are XORed into the slot behind its twelve header bytes */
extern "C" __global__ void __launch_bounds__(LC3FEC_THREADS) lc3_fec_rec_bytes_kernel(lc3fec_rec_io q, const int32_t* __restrict__ table)
{
    enum { PER = LC3FEC_THREADS / LC3FEC_REC_LANES };
    __shared__ long long sh_at[PER][LC3FEC_MAX_BITS];
    __shared__ int32_t sh_len[PER][LC3FEC_MAX_BITS];
    const int l = threadIdx.x & (LC3FEC_REC_LANES - 1), slot = threadIdx.x / LC3FEC_REC_LANES;
    const long long f = (long long)blockIdx.x * PER + slot;
    const int32_t size = f < q.n_fec ? q.rec_dg_sizes[f] : 0;         /* the same in every lane of the wave */
    lc3fec_item h;
    h.plen = 0; h.hl = 0; h.mask = 0; h.sn = 0;
    if (size > 0) {
        lc3fec_item_header(&q, f, &h);                                /* 0: the verdict has said so */
        if (l < LC3FEC_MAX_BITS) {
            long long at = 0;
            int32_t len = -1;
            if (h.mask >> (LC3FEC_MAX_BITS - 1 - l) & 1) {
                if (!lc3fec_lookup(&q, table, q.fec_stream[f], (h.sn + (uint32_t)l) & 0xFFFFu, &at, &len)) len = -1;
                else if (len > (int32_t)h.plen) len = (int32_t)h.plen;
            }
            sh_at[slot][l] = at; sh_len[slot][l] = len;
        }
    }
    __syncthreads();
    if (size > 0)
        lc3fec_xor_store<LC3FEC_REC_LANES>((uintptr_t)q.ring + (uintptr_t)(q.rec_offset + f * q.rec_stride + LC3R_FIXED), size - LC3R_FIXED, (uintptr_t)q.ring, sh_at[slot],
                                           sh_len[slot], h.hl == LC3FEC_HEADER ? 16 : LC3FEC_MAX_BITS, (uintptr_t)q.ring + (uintptr_t)(q.fec_offsets[f] + h.hl), (int32_t)h.plen, l);
}
