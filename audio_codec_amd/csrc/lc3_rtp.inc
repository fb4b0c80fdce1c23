/* lc3_rtp.inc -- the RTP framing kernels (included by lc3_rtp.hip): received datagrams -> the item arrays of the probe and the ingest, and the egress's packet
 * list -> RTP headers in the header rooms of the wire buffer, by the rules of include/lc3plus_batch.h "RTP framing" (lc3_rtp_shim.h holds their text, shared
 * with lc3plus_plan_rtp_parse and lc3plus_plan_rtp_stamp on the host).  Every offset into the ring and the wire buffer is 64 bits wide. */

/* zeroes the parse call's stats in front of the parse kernel */
extern "C" __global__ void __launch_bounds__(WAVE) lc3_rtp_fill_kernel(int32_t* __restrict__ stats)
{
    if (threadIdx.x < LC3R_STATS_WORDS) stats[threadIdx.x] = 0;
}

/* One datagram per lane, grid-stride.  The SSRC table is staged in LDS where the launch gives it room (lds_entries = n_ssrc, else 0: the lanes then search it in
 * global memory).  Of a datagram a lane reads its first twelve bytes as three or four aligned words, the extension's length and the last byte as one aligned
 * word each (two where the length's bytes lie on both sides of a word boundary).  stats: every wave tallies its items per status over its whole walk - lane k
 * keeps the count of status k; the waves of a workgroup add their counts in LDS, and the workgroup adds the sums with one vector atomic at its end.  (One
 * atomic per wave was measured first: 4 096 waves adding to the same two words took 50 us, the atomics one behind the other - DESIGN 10i.) */
extern "C" __global__ void __launch_bounds__(LC3R_PARSE_THREADS) lc3_rtp_parse_kernel(const uint8_t* __restrict__ ring, long long capacity, const long long* __restrict__ dg_offsets,
                                                                        const int32_t* __restrict__ dg_sizes, long long n_items, const int32_t* __restrict__ ssrc_key,
                                                                        const int32_t* __restrict__ ssrc_stream, int n_ssrc, int lds_entries, int n_streams,
                                                                        const int32_t* __restrict__ payload_type, int payload_room, lc3r_items out,
                                                                        int32_t* __restrict__ stats)
{
    extern __shared__ int32_t lc3r_table[];                          /* lds_entries keys, then lds_entries streams */
    __shared__ int lc3r_tally[LC3R_STATUSES];
    if (threadIdx.x < LC3R_STATUSES) lc3r_tally[threadIdx.x] = 0;     /* the barrier in front of its first use is the one behind the walk */
    const int32_t* key = ssrc_key;
    const int32_t* strm = ssrc_stream;
    if (lds_entries > 0) {                                           /* every load of a lane's share is issued before the first is waited for */
        enum { SHARE = LC3R_LDS_ENTRIES / LC3R_PARSE_THREADS };
        int32_t k_[SHARE], s_[SHARE];
#pragma unroll
        for (int j = 0; j < SHARE; j++) {
            const int k = threadIdx.x + j * LC3R_PARSE_THREADS;
            k_[j] = k < lds_entries ? ssrc_key[k] : 0; s_[j] = k < lds_entries ? ssrc_stream[k] : 0;
        }
#pragma unroll
        for (int j = 0; j < SHARE; j++) {
            const int k = threadIdx.x + j * LC3R_PARSE_THREADS;
            if (k < lds_entries) { lc3r_table[k] = k_[j]; lc3r_table[lds_entries + k] = s_[j]; }
        }
        __syncthreads();
        key = lc3r_table; strm = lc3r_table + lds_entries;
    }
    const int lane = threadIdx.x & (WAVE - 1);
    const long long stride = (long long)gridDim.x * LC3R_PARSE_THREADS;
    int tally = 0;
    for (long long i0 = (long long)blockIdx.x * LC3R_PARSE_THREADS + (threadIdx.x - lane); i0 < n_items; i0 += stride) {      /* i0: the same in every lane of a wave */
        const long long i = i0 + lane;
        int st = -1;
        if (i < n_items) {
            const lc3r_item it = lc3r_parse(ring, capacity, dg_offsets[i], dg_sizes[i], key, strm, n_ssrc, n_streams, payload_type, payload_room);
            lc3r_item_out(&out, i, &it);
            st = it.status;
        }
        if (stats)
            for (int k = 0; k < LC3R_STATUSES; k++) {
                const int c = __popcll(__ballot(st == k));
                if (lane == k) tally += c;
            }
    }
    if (stats) {
        __syncthreads();
        if (lane < LC3R_STATUSES && tally) atomicAdd(&lc3r_tally[lane], tally);
        __syncthreads();
        if (threadIdx.x < LC3R_STATUSES && lc3r_tally[threadIdx.x]) atomicAdd(stats + threadIdx.x, lc3r_tally[threadIdx.x]);
    }
}

/* One packet per lane, grid-stride over the packets in front of *n_packets, which is read here as the egress's copy kernel reads it.  A packet the rule refuses
 * writes nothing but its status */
extern "C" __global__ void __launch_bounds__(LC3R_THREADS) lc3_rtp_stamp_kernel(lc3r_stamp_in q, long long max_packets, const long long* __restrict__ n_packets,
                                                                        uint8_t* __restrict__ wire, uint8_t* __restrict__ pkt_status)
{
    long long n = *n_packets;
    if (n > max_packets) n = max_packets;
    const long long stride = (long long)gridDim.x * LC3R_THREADS;
    for (long long p = (long long)blockIdx.x * LC3R_THREADS + threadIdx.x; p < n; p += stride) {
        uint32_t hdr[3];
        long long at = 0;
        const int st = lc3r_stamp(&q, p, hdr, &at);
        if (st == LC3R_STAMPED) lc3r_header_out(wire, at, hdr);
        if (pkt_status) pkt_status[p] = (uint8_t)st;
    }
}

/* one route per lane: next_ts and next_resume */
extern "C" __global__ void __launch_bounds__(LC3R_THREADS) lc3_rtp_route_kernel(lc3r_stamp_in q, int32_t* __restrict__ next_ts, uint8_t* __restrict__ next_resume)
{
    const long long r = (long long)blockIdx.x * LC3R_THREADS + threadIdx.x;
    if (r < q.n_routes) lc3r_route_out(&q, (int)r, next_ts, next_resume);
}
