/* lc3_gcm.inc -- the kernels of Secure RTP with AES-GCM (included by lc3_gcm.hip): the stamp's packets -> SRTP packets with a 16-byte tag in a destination buffer,
 * and received ones -> authenticated, decrypted RTP datagrams in place with the replay state advanced, by the rules of include/lc3plus_batch.h "Secure RTP,
 * AEAD" (lc3_gcm_shim.h holds their text, shared with lc3plus_plan_srtp_gcm_protect and lc3plus_plan_srtp_gcm_unprotect on the host).
 *
 * The split is the SRTP library's: one packet per lane, the list walked grid-stride, 256 lanes a workgroup, Te0 computed into LDS by every workgroup, round
 * keys, salt and round count read from the route's or source's context where it lies, so that contexts of both key sizes stand side by side.  GHASH is serial
 * inside a packet like SHA-1, 32 table steps a block.  Protect is one walk: fetch, XOR, hash the ciphertext word, store.  Unprotect is two: hash without a store,
 * compare, then decrypt into the sink.  The lanes of a wave hold different keys, so different GHASH tables: every lane copies its table (256 bytes of its
 * context) into LDS before its walk, lane-interleaved so that the lanes of a wave read 64 different banks - 64 KiB a workgroup, two workgroups a CU.  With
 * -DLC3G_LDS_TABLE=0 the table is read from the context in global memory instead, 16 bytes a step; that build measured 1.5 to 1.6 times slower (the
 * comparison of DESIGN 10l, profiles/gcm_tables_ab.txt).  The five bookkeeping kernels are the SRTP library's over the same shared functions under names of this library's own: that code object stays
 * as it is. */

/* Te0 into LDS */
static inline __device__ void lc3g_tables(uint32_t* te)
{
    if (threadIdx.x < LC3S_TE_WORDS) te[threadIdx.x] = lc3s_te0(threadIdx.x);
    __syncthreads();
}
#if LC3G_LDS_TABLE
#define LC3G_TAB_DECL __shared__ uint32_t gtab[64 * LC3S_THREADS];
#define LC3G_TAB (gtab + threadIdx.x)
#define LC3G_TS LC3S_THREADS
/* word w of entry e of this lane's table goes to word (4 e + w) * 256 + lane: only this lane reads or writes it, so no barrier */
static inline __device__ void lc3g_table_in(uint32_t* gtab, const uint32_t* ctx)
{
    for (int i = 0; i < 64; i++) gtab[i * LC3S_THREADS + threadIdx.x] = ctx[LC3G_CTX_TABLE + i];
}
#else
#define LC3G_TAB_DECL
#define LC3G_TAB ((const uint32_t*)0)
#define LC3G_TS 1
#endif

/* One packet per lane, grid-stride over the packets in front of *n_packets, which is read here as the stamp's kernel reads it */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_gcm_protect_kernel(lc3s_protect_in q, long long max_packets, const long long* __restrict__ n_packets,
                                                                       long long* __restrict__ out_offset, int32_t* __restrict__ out_size,
                                                                       uint8_t* __restrict__ out_status)
{
    __shared__ uint32_t te[LC3S_TE_WORDS];
    LC3G_TAB_DECL
    lc3g_tables(te);
    long long n = *n_packets;
    if (n > max_packets) n = max_packets;
    const long long stride = (long long)gridDim.x * LC3S_THREADS;
    for (long long p = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x; p < n; p += stride) {
        int32_t size = 0;
#if LC3G_LDS_TABLE
        const int r = q.route[p];
        if (r >= 0 && r < q.n_routes) lc3g_table_in(gtab, (const uint32_t*)q.ctx + (size_t)r * LC3G_CTX_WORDS);
#endif
        const int st = lc3g_protect(&q, p, te, 1, LC3G_TAB, LC3G_TS, &size);
        out_offset[p] = p * q.dst_stride; out_size[p] = size; out_status[p] = (uint8_t)st;
    }
}

/* one route per lane: next_roc */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_gcm_route_kernel(lc3s_protect_in q, int32_t* __restrict__ next_roc)
{
    const long long r = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x;
    if (r < q.n_routes) lc3s_route_out(&q, (int)r, next_roc);
}

/* the workspace's arrays of an unprotect call (lc3_srtp_shim.h) */
struct lc3g_work { unsigned long long* top1; unsigned long long* bits; long long* accepted; int32_t* first; int32_t* src; };

/* one source per lane: nothing accepted, no first item; the first lanes zero the stats */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_gcm_init_kernel(lc3g_work w, int n_ssrc, int32_t* __restrict__ stats)
{
    const long long s = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x;
    if (stats && s < LC3S_STATS_WORDS) stats[s] = 0;
    if (s < n_ssrc) { w.top1[s] = 0; w.bits[s] = 0; w.first[s] = 0x7FFFFFFF; }
}

/* One item per lane, grid-stride: checks 1 and 2 with a tag of 16 bytes.  Leaves the item's source, or -1 - its status, and for a source that has not started
 * the smallest list index among its items (a vector atomic minimum) */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_gcm_scan_kernel(lc3srtp_unprotect_call q, lc3g_work w)
{
    const long long stride = (long long)gridDim.x * LC3S_THREADS;
    for (long long i = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x; i < q.n_items; i += stride) {
        const lc3s_item it = lc3s_check((const uint8_t*)q.ring, q.ring_capacity, q.dg_offsets[i], q.dg_sizes[i], LC3G_TAG_BYTES, q.ssrc_key, q.n_ssrc);
        w.src[i] = it.status == LC3S_OK ? it.src : -1 - (int32_t)it.status;
        if (it.status == LC3S_OK && !(q.state_in[(size_t)it.src * LC3S_STATE_WORDS + LC3S_FLAGS] & LC3S_STARTED)) atomicMin(&w.first[it.src], (int32_t)i);
    }
}

/* One item per lane, grid-stride: checks 3 to 6 against state_in - the hash, the comparison, the decryption in place; sizes_out, status, index; the source's
 * largest accepted index by a 64-bit vector atomic maximum.  stats: every lane adds to its workgroup's tally in LDS, the workgroup adds its sums with one
 * vector atomic per status at its end */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_gcm_auth_kernel(lc3srtp_unprotect_call q, lc3g_work w)
{
    __shared__ uint32_t te[LC3S_TE_WORDS];
    __shared__ int tally[LC3S_STATUSES];
    LC3G_TAB_DECL
    if (threadIdx.x < LC3S_STATUSES) tally[threadIdx.x] = 0;
    lc3g_tables(te);
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
            const lc3s_item it = lc3s_check(ring, q.ring_capacity, off, size, LC3G_TAG_BYTES, q.ssrc_key + s, 1);      /* the header again; the source is known */
            const int32_t* state = q.state_in + (size_t)s * LC3S_STATE_WORDS;
            const uint32_t* ctx = (const uint32_t*)q.ctx + (size_t)s * LC3G_CTX_WORDS;
            uint32_t s_l_first = 0;
            if (!(state[LC3S_FLAGS] & LC3S_STARTED)) s_l_first = lc3s_seq_at(ring, q.dg_offsets[w.first[s]]);
            lc3s_item me = it;
            me.src = s;
#if LC3G_LDS_TABLE
            lc3g_table_in(gtab, ctx);
#endif
            st = lc3g_unprotect(ring, off, size, &me, state, s_l_first, ctx, te, 1, LC3G_TAB, LC3G_TS, &index);
            if (st == LC3S_OK) {
                size_out = size - LC3G_TAG_BYTES; accepted = index;
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
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_gcm_window_kernel(lc3srtp_unprotect_call q, lc3g_work w)
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
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) lc3_gcm_state_kernel(lc3srtp_unprotect_call q, lc3g_work w)
{
    const long long s = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x;
    if (s < q.n_ssrc) lc3s_state_out(q.state_in + (size_t)s * LC3S_STATE_WORDS, q.state_out + (size_t)s * LC3S_STATE_WORDS, w.top1[s], w.bits[s]);
}
