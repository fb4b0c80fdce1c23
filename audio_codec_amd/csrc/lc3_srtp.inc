/* lc3_srtp.inc -- the Secure RTP kernels (included by lc3_srtp.hip): the stamp's packets -> SRTP packets in a destination buffer, and received SRTP datagrams ->
 * authenticated, decrypted RTP datagrams in place with the replay state advanced, by the rules of include/lc3plus_batch.h "Secure RTP" (lc3_srtp_shim.h holds
 * their text, shared with lc3plus_plan_srtp_protect and lc3plus_plan_srtp_unprotect on the host).
 *
 * The split: one packet per lane.  SHA-1 is serial inside a packet and the keystream blocks feed it in order, so a lane walks its packet once, word by word:
 * fetch, XOR, store, and every sixteen words one compression whose 80 rounds are unrolled over a schedule in registers.  The parallelism is that of the list
 * (a call of 4 096 x 64 packets is 4 096 waves), not of the packet.  The AES table is computed into LDS by the first 256 lanes of every workgroup; LC3S_NT is
 * the number of tables kept there, 1 (Te0, the others by rotation) in the product, 4 in a build for the comparison.  Round keys, salt and midstates are read from the route's context where it lies: the lanes
 * of a wave mostly share a route or walk neighbouring ones. */

/* Te0, or Te0 .. Te3, into LDS */
static inline __device__ void lc3s_tables(uint32_t* te)
{
    if (threadIdx.x < LC3S_TE_WORDS) {
        const uint32_t v = lc3s_te0(threadIdx.x);
        te[threadIdx.x] = v;
        if (LC3S_NT == 4)
            for (int k = 1; k < 4; k++) te[k * LC3S_TE_WORDS + threadIdx.x] = v >> (8 * k) | v << (32 - 8 * k);
    }
    __syncthreads();
}

/* One packet per lane, grid-stride over the packets in front of *n_packets, which is read here as the stamp's kernel reads it */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_srtp_protect_kernel(lc3s_protect_in q, long long max_packets, const long long* __restrict__ n_packets,
                                                                        long long* __restrict__ out_offset, int32_t* __restrict__ out_size,
                                                                        uint8_t* __restrict__ out_status)
{
    __shared__ uint32_t te[LC3S_NT * LC3S_TE_WORDS];
    lc3s_tables(te);
    long long n = *n_packets;
    if (n > max_packets) n = max_packets;
    const long long stride = (long long)gridDim.x * LC3S_THREADS;
    for (long long p = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x; p < n; p += stride) {
        int32_t size = 0;
        const int st = lc3s_protect(&q, p, te, LC3S_NT, &size);
        out_offset[p] = p * q.dst_stride; out_size[p] = size; out_status[p] = (uint8_t)st;
    }
}

/* one route per lane: next_roc */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_srtp_route_kernel(lc3s_protect_in q, int32_t* __restrict__ next_roc)
{
    const long long r = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x;
    if (r < q.n_routes) lc3s_route_out(&q, (int)r, next_roc);
}

/* the workspace's arrays of an unprotect call (lc3_srtp_shim.h) */
struct lc3s_work { unsigned long long* top1; unsigned long long* bits; long long* accepted; int32_t* first; int32_t* src; };

/* one source per lane: nothing accepted, no first item; the first lanes zero the stats */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_srtp_init_kernel(lc3s_work w, int n_ssrc, int32_t* __restrict__ stats)
{
    const long long s = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x;
    if (stats && s < LC3S_STATS_WORDS) stats[s] = 0;
    if (s < n_ssrc) { w.top1[s] = 0; w.bits[s] = 0; w.first[s] = 0x7FFFFFFF; }
}

/* One item per lane, grid-stride: checks 1 and 2.  Leaves the item's source, or -1 - its status, and for a source that has not started the smallest list index
 * among its items (a vector atomic minimum) */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_srtp_scan_kernel(lc3srtp_unprotect_call q, lc3s_work w)
{
    const long long stride = (long long)gridDim.x * LC3S_THREADS;
    for (long long i = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x; i < q.n_items; i += stride) {
        const lc3s_item it = lc3s_check((const uint8_t*)q.ring, q.ring_capacity, q.dg_offsets[i], q.dg_sizes[i], q.tag_len, q.ssrc_key, q.n_ssrc);
        w.src[i] = it.status == LC3S_OK ? it.src : -1 - (int32_t)it.status;
        if (it.status == LC3S_OK && !(q.state_in[(size_t)it.src * LC3S_STATE_WORDS + LC3S_FLAGS] & LC3S_STARTED)) atomicMin(&w.first[it.src], (int32_t)i);
    }
}

/* One item per lane, grid-stride: checks 3 to 6 against state_in, the authentication, the decryption in place; sizes_out, status, index; the source's largest
 * accepted index by a 64-bit vector atomic maximum.  stats: every lane adds to its workgroup's tally in LDS, the workgroup adds its sums with one vector atomic
 * per status at its end (as the parse does) */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_srtp_auth_kernel(lc3srtp_unprotect_call q, lc3s_work w)
{
    __shared__ uint32_t te[LC3S_NT * LC3S_TE_WORDS];
    __shared__ int tally[LC3S_STATUSES];
    if (threadIdx.x < LC3S_STATUSES) tally[threadIdx.x] = 0;
    lc3s_tables(te);
    uint8_t* ring = (uint8_t*)q.ring;
    const long long stride = (long long)gridDim.x * LC3S_THREADS;
    for (long long i = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x; i < q.n_items; i += stride) {
        const int s = w.src[i];
        int st = -1 - s;
        long long index = 0, accepted = -1;
        int32_t size_out = 0;
        if (s >= 0) {
            const long long off = q.dg_offsets[i];
            const int32_t size = q.dg_sizes[i];
            const lc3s_item it = lc3s_check(ring, q.ring_capacity, off, size, q.tag_len, q.ssrc_key + s, 1);      /* the header again; the source is known */
            const int32_t* state = q.state_in + (size_t)s * LC3S_STATE_WORDS;
            uint32_t s_l_first = 0;
            if (!(state[LC3S_FLAGS] & LC3S_STARTED)) s_l_first = lc3s_seq_at(ring, q.dg_offsets[w.first[s]]);
            lc3s_item me = it;
            me.src = s;
            st = lc3s_unprotect(ring, off, size, q.tag_len, &me, state, s_l_first, (const uint32_t*)q.ctx + (size_t)s * LC3S_CTX_WORDS, te, LC3S_NT, &index);
            if (st == LC3S_OK) {
                size_out = size - q.tag_len; accepted = index;
                atomicMax(&w.top1[s], (unsigned long long)index + 1ull);
            }
        }
        w.accepted[i] = accepted;
        q.sizes_out[i] = size_out;
        if (q.status) q.status[i] = (uint8_t)st;
        if (q.index) q.index[i] = index;
        if (q.stats) atomicAdd(&tally[st], 1);
    }
    if (q.stats) {
        __syncthreads();
        if (threadIdx.x < LC3S_STATUSES && tally[threadIdx.x]) atomicAdd(q.stats + threadIdx.x, tally[threadIdx.x]);
    }
}

/* One item per lane, grid-stride, once every maximum stands: the window bit of every accepted item against its source's new top, by a 64-bit vector atomic OR */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_srtp_window_kernel(lc3srtp_unprotect_call q, lc3s_work w)
{
    const long long stride = (long long)gridDim.x * LC3S_THREADS;
    for (long long i = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x; i < q.n_items; i += stride) {
        const long long index = w.accepted[i];
        if (index < 0) continue;
        const int s = w.src[i];
        const unsigned long long bit = lc3s_window_bit(q.state_in + (size_t)s * LC3S_STATE_WORDS, w.top1[s], index);
        if (bit) atomicOr(&w.bits[s], bit);
    }
}

/* one source per lane: state_out (which may be state_in: a lane reads its block before it writes it, and no other lane touches it) */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_srtp_state_kernel(lc3srtp_unprotect_call q, lc3s_work w)
{
    const long long s = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x;
    if (s < q.n_ssrc) lc3s_state_out(q.state_in + (size_t)s * LC3S_STATE_WORDS, q.state_out + (size_t)s * LC3S_STATE_WORDS, w.top1[s], w.bits[s]);
}
