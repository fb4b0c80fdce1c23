/* lc3_rtcp.inc -- the reception report kernels (included by lc3_rtcp.hip): the parse's item arrays, an arrival time per item and a state block per stream ->
 * the advanced state, the RR report blocks and a status per item, by the rule of include/lc3plus_batch.h "Reception reports" (lc3_rtcp_shim.h holds its text,
 * shared with lc3plus_plan_rtcp_stats on the host).  The list interleaves the streams and the rule is serial inside a stream, in list order: count the items of
 * each stream, scan the counts, bring each stream's item indices together, sort them where the placement was not in order, walk them. */

/* zeroes the counts and the number of long streams in front of the count kernel: cur [n_streams] and nbig lie one behind the other */
extern "C" __global__ void __launch_bounds__(LC3Q_THREADS) lc3_rtcp_fill_kernel(int32_t* __restrict__ cur, long long n)
{
    const long long stride = (long long)gridDim.x * LC3Q_THREADS;
    for (long long k = (long long)blockIdx.x * LC3Q_THREADS + threadIdx.x; k < n; k += stride) cur[k] = 0;
}

/* The lanes of a wave whose items belong to one stream and lie side by side form a run: -> the run's first lane, *len its length.  Every lane of the wave
 * must call this.  In a list in arrival order nearly every lane is a run of its own; in a list that holds each sender's burst in one piece a wave holds one run or
 * two, and 64 atomics on one word - which the memory system takes one behind the other - become one */
static __device__ int lc3q_run(int s, int lane, int* len)
{
    const int prev = __shfl_up(s, 1);
    const unsigned long long heads = __ballot(lane == 0 || s != prev), upto = (2ull << lane) - 1ull;      /* lane 63: 2 << 63 is 0, upto all ones */
    const int head = 63 - (int)__clzll(heads & upto);
    const unsigned long long above = heads & ~upto;
    *len = (above ? (int)__builtin_ctzll(above) : WAVE) - head;
    return head;
}

/* One item per lane, grid-stride: cur[s] += the run's length, by the first lane of every run of a valid stream */
extern "C" __global__ void __launch_bounds__(LC3Q_THREADS) lc3_rtcp_count_kernel(const int32_t* __restrict__ stream, long long n_items, int n_streams,
                                                                                int32_t* __restrict__ cur)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long stride = (long long)gridDim.x * LC3Q_THREADS;
    for (long long i0 = (long long)blockIdx.x * LC3Q_THREADS + (threadIdx.x - lane); i0 < n_items; i0 += stride) {      /* i0: the same in every lane of a wave */
        const long long i = i0 + lane;
        int s = -1;
        if (i < n_items) { s = stream[i]; if (s >= n_streams) s = -1; }
        int len;
        const int head = lc3q_run(s, lane, &len);
        if (lane == head && s >= 0) atomicAdd(cur + s, len);
    }
}

/* One workgroup: the exclusive scan of the counts into off, the cursors set to it, and the list of the streams with more than LC3Q_LDS_ITEMS items (in any
 * order: each is placed and walked on its own) */
extern "C" __global__ void __launch_bounds__(LC3Q_SCAN_THREADS) lc3_rtcp_scan_kernel(int32_t* __restrict__ off, int32_t* __restrict__ cur, int32_t* __restrict__ nbig,
                                                                                    int32_t* __restrict__ big, int n_streams, int most_big)
{
    __shared__ int wsum[LC3Q_SCAN_THREADS / WAVE];
    __shared__ int carry;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (long long s0 = 0; s0 < n_streams; s0 += LC3Q_SCAN_THREADS) {
        const long long s = s0 + threadIdx.x;
        const int c = s < n_streams ? cur[s] : 0;
        int incl = c;
        for (int d = 1; d < WAVE; d <<= 1) { const int o = __shfl_up(incl, d); if (lane >= d) incl += o; }
        if (lane == WAVE - 1) wsum[wave] = incl;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; w++) before += wsum[w];
        if (s < n_streams) {
            const int at = before + incl - c;
            off[s] = at; cur[s] = at;
            if (c > LC3Q_LDS_ITEMS) { const int k = atomicAdd(nbig, 1); if (k < most_big) big[k] = (int)s; }
        }
        __syncthreads();
        if (threadIdx.x == LC3Q_SCAN_THREADS - 1) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[n_streams] = carry;
}

/* One item per lane, grid-stride.  An item of no stream is DROPPED here and now.  A run (lc3q_run) of a stream with at most LC3Q_LDS_ITEMS items takes the next
 * places of its stream's segment, in whatever order the runs arrive: the walk sorts the segment.  The items of a longer stream are left to the place kernel */
extern "C" __global__ void __launch_bounds__(LC3Q_THREADS) lc3_rtcp_scatter_kernel(const int32_t* __restrict__ stream, long long n_items, int n_streams,
                                                                                  const int32_t* __restrict__ off, int32_t* __restrict__ cur, int32_t* __restrict__ idx,
                                                                                  int32_t* __restrict__ ext_seq, uint8_t* __restrict__ item_status)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long stride = (long long)gridDim.x * LC3Q_THREADS;
    for (long long i0 = (long long)blockIdx.x * LC3Q_THREADS + (threadIdx.x - lane); i0 < n_items; i0 += stride) {      /* i0: the same in every lane of a wave */
        const long long i = i0 + lane;
        int s = -1;
        if (i < n_items) {
            s = stream[i];
            if (s < 0 || s >= n_streams) {
                s = -1;
                if (item_status) item_status[i] = LC3Q_DROPPED;
                if (ext_seq) ext_seq[i] = 0;
            }
        }
        int len, end = 0, first = 0;
        const int head = lc3q_run(s, lane, &len);
        bool place = false;
        if (s >= 0) { end = off[s + 1]; place = end - off[s] <= LC3Q_LDS_ITEMS; }
        if (lane == head && place) first = atomicAdd(cur + s, len);
        const int at = __shfl(first, head) + lane - head;
        if (place && at < end) idx[at] = (int32_t)i;                 /* at < end always, while the list is what the count kernel read */
    }
}

/* One workgroup per long stream, grid-stride over the list the scan made: the workgroup reads the whole item list in order, 1 024 items a round, and writes the
 * indices of its stream's items into the stream's segment in that order (a ballot per wave, the waves' counts through LDS) */
extern "C" __global__ void __launch_bounds__(LC3Q_PLACE_THREADS) lc3_rtcp_place_kernel(const int32_t* __restrict__ stream, long long n_items,
                                                                                      const int32_t* __restrict__ off, const int32_t* __restrict__ nbig,
                                                                                      const int32_t* __restrict__ big, int most_big, int32_t* __restrict__ idx)
{
    __shared__ int wcnt[LC3Q_PLACE_THREADS / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int n = *nbig;
    if (n > most_big) n = most_big;
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const int s = big[k], beg = off[s], len = off[s + 1] - beg;
        int done = 0;                                                /* the same in every lane */
        for (long long i0 = 0; i0 < n_items; i0 += LC3Q_PLACE_THREADS) {
            const long long i = i0 + threadIdx.x;
            const bool mine = i < n_items && stream[i] == s;
            const unsigned long long m = __ballot(mine);
            if (lane == 0) wcnt[wave] = (int)__popcll(m);
            __syncthreads();
            int before = 0, all = 0;
            for (int w = 0; w < LC3Q_PLACE_THREADS / WAVE; w++) { const int c = wcnt[w]; if (w < wave) before += c; all += c; }
            const int at = done + before + (int)__popcll(m & ((1ull << lane) - 1ull));
            if (mine && at < len) idx[beg + at] = (int32_t)i;
            done += all;
            __syncthreads();
        }
    }
}

/* 64 values, one per lane, ascending by lane: a bitonic network of 21 exchanges */
static __device__ int lc3q_sort_wave(int v, int lane)
{
    for (int k = 2; k <= WAVE; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int o = __shfl_xor(v, j);
            const bool low = !(lane & j), up = !(lane & k);
            v = low == up ? (v < o ? v : o) : (v > o ? v : o);
        }
    return v;
}
/* p values in LDS (p a power of two, 128 ... LC3Q_LDS_ITEMS), ascending: the same network, every lane p / 128 pairs per exchange */
static __device__ void lc3q_sort_lds(int* seg, int p, int lane)
{
    for (int k = 2; k <= p; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < p / 2; t += WAVE) {
                const int a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const int va = seg[a], vb = seg[b];
                if ((va > vb) == !(a & k)) { seg[a] = vb; seg[b] = va; }
            }
            __syncthreads();
        }
}

/* One wave (a workgroup of its own) per stream, grid-stride.  The stream's item indices: up to 64 sorted in registers, up to LC3Q_LDS_ITEMS sorted in LDS, more
 * than that read in the order the place kernel wrote them.  64 items a round: the lanes gather seq, timestamp and arrival and compute the transits, then the
 * rule runs item by item on values every lane holds alike (v_readlane of the round's lanes), and the lanes scatter their items' status and ext_seq.  The state,
 * the stats and the block go out once, as vector stores of lane 0 */
extern "C" __global__ void __launch_bounds__(LC3Q_WALK_THREADS) lc3_rtcp_walk_kernel(lc3rtcp_stats_call q, const int32_t* __restrict__ off, const int32_t* __restrict__ idx)
{
    __shared__ int seg[LC3Q_LDS_ITEMS];
    const int lane = threadIdx.x;
    for (long long s = blockIdx.x; s < q.n_streams; s += gridDim.x) {
        const int beg = off[s], len = off[s + 1] - beg;
        lc3q_state st;
        for (int k = 0; k < LC3Q_STATE_WORDS; k++) st.w[k] = (uint32_t)q.state_in[s * LC3Q_STATE_WORDS + k];
        int mine = 0x7FFFFFFF;
        if (len <= LC3Q_WAVE_ITEMS) {
            if (lane < len) mine = idx[beg + lane];
            if (len > 1) mine = lc3q_sort_wave(mine, lane);
        } else if (len <= LC3Q_LDS_ITEMS) {
            int p = 2 * WAVE;
            while (p < len) p <<= 1;
            for (int t = lane; t < p; t += WAVE) seg[t] = t < len ? idx[beg + t] : 0x7FFFFFFF;
            __syncthreads();
            lc3q_sort_lds(seg, p, lane);
        }
        int tally[LC3Q_STATS_WORDS] = {0, 0, 0, 0};
        for (int c = 0; c < len; c += WAVE) {
            const int n = len - c < WAVE ? len - c : WAVE;
            int i = -1;
            if (lane < n) i = len <= LC3Q_WAVE_ITEMS ? mine : len <= LC3Q_LDS_ITEMS ? seg[c + lane] : idx[beg + c + lane];
            if (i >= q.n_items) i = -1;                              /* never, while the list is what the count kernel read */
            uint32_t sq = 0, tr = 0;
            if (i >= 0) { sq = (uint32_t)q.seq[i]; tr = (uint32_t)q.arrival[i] - (uint32_t)q.timestamp[i]; }
            int my_status = 0;
            uint32_t my_ext = 0;
            for (int j = 0; j < n; j++) {
                uint32_t ext;
                const int r = lc3q_step(&st, (uint32_t)__builtin_amdgcn_readlane((int)sq, j), (uint32_t)__builtin_amdgcn_readlane((int)tr, j), &ext);
                if (lane == j) { my_status = r; my_ext = ext; }
                tally[LC3Q_ST_COUNTED] += r != LC3Q_JUMP; tally[LC3Q_ST_JUMP] += r == LC3Q_JUMP; tally[LC3Q_ST_RESTART] += r == LC3Q_RESTART;
                tally[LC3Q_ST_REORDERED] += r == LC3Q_REORDERED;
            }
            if (i >= 0) {
                if (q.item_status) q.item_status[i] = (uint8_t)my_status;
                if (q.ext_seq) q.ext_seq[i] = (int32_t)my_ext;
            }
        }
        uint32_t blk[LC3Q_BLOCK_WORDS];
        if (q.make_report) lc3q_report(&st, (uint32_t)q.ssrc[s], q.lsr ? (uint32_t)q.lsr[s] : 0u, q.dlsr ? (uint32_t)q.dlsr[s] : 0u, blk);
        if (lane == 0) {
            for (int k = 0; k < LC3Q_STATE_WORDS; k++) q.state_out[s * LC3Q_STATE_WORDS + k] = (int32_t)st.w[k];
            if (q.stream_stats) for (int k = 0; k < LC3Q_STATS_WORDS; k++) q.stream_stats[s * LC3Q_STATS_WORDS + k] = tally[k];
            if (q.make_report) lc3q_block_out(q.blocks + s * LC3Q_BLOCK_BYTES, blk);
        }
        __syncthreads();                                             /* seg is the next stream's */
    }
}
