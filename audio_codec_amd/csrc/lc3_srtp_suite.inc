/* lc3_srtp_suite.inc -- the seven kernels of a Secure RTP suite and the host code that launches them, one text for every suite's sibling library (lc3_srtp.hip:
 * AES-CM with HMAC-SHA1; lc3_gcm.hip: AES-GCM): the stamp's packets -> SRTP packets in a destination buffer, and received SRTP datagrams -> authenticated,
 * decrypted RTP datagrams in place with the replay state advanced, by the rules of include/lc3plus_batch.h "Secure RTP" and "Secure RTP, AEAD" (lc3_srtp_shim.h
 * and lc3_gcm_shim.h hold their text, shared with the lc3plus_plan_srtp_* functions on the host).  A library defines its suite and includes this file once:
 *     SUITE_KERNEL(x)    the name of kernel x: lc3_NAME_x_kernel          SUITE_ABI(x)      the exported name of host function x: lc3NAME_x
 *     SIB_NAME           the prefix of the library's messages (lc3_sibling.h)
 *     SUITE_TAG(q)       the tag's length in a kernel, q the call by value   SUITE_TAG_OK(t)   whether the suite takes a call whose tag_len is t
 *     SUITE_CTX_WORDS    the words of a route's or source's context
 *     SUITE_LDS          the declarations in LDS of a kernel that runs a rule: te, and what else the rule reads there
 *     SUITE_TABLES()     fills te, with the barrier behind it
 *     SUITE_LANE(ctx)    what a lane does with its context in front of the rule
 *     SUITE_PROTECT(q, p, size)   SUITE_UNPROTECT(ring, off, size, it, state, s_l_first, ctx, index)    the one call to each rule; q is the kernel's
 *
 * The split: one packet per lane.  The hash of either suite is serial inside a packet and the keystream blocks feed it in order, so a lane walks its packet
 * word by word: fetch, XOR, store, hash.  The parallelism is that of the list (a call of 4 096 x 64 packets is 4 096 waves), not of the packet.  Every workgroup
 * computes the AES table into LDS; round keys and salt are read from the route's or source's context where it lies: the lanes of a wave mostly share a route or
 * walk neighbouring ones.  The library keeps no state but its launch counts, no key, and allocates nothing: all scratch lies in the caller's workspace. */

/* One packet per lane, grid-stride over the packets in front of *n_packets, which is read here as the stamp's kernel reads it */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) SUITE_KERNEL(protect)(lc3s_protect_in q, long long max_packets, const long long* __restrict__ n_packets,
                                                                      long long* __restrict__ out_offset, int32_t* __restrict__ out_size,
                                                                      uint8_t* __restrict__ out_status)
{
    SUITE_LDS
    SUITE_TABLES();
    long long n = *n_packets;
    if (n > max_packets) n = max_packets;
    const long long stride = (long long)gridDim.x * LC3S_THREADS;
    for (long long p = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x; p < n; p += stride) {
        int32_t size = 0;
        const int r = q.route[p];
        if (r >= 0 && r < q.n_routes) SUITE_LANE((const uint32_t*)q.ctx + (size_t)r * SUITE_CTX_WORDS);
        const int st = SUITE_PROTECT(&q, p, &size);
        out_offset[p] = p * q.dst_stride; out_size[p] = size; out_status[p] = (uint8_t)st;
    }
}

/* one route per lane: next_roc */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) SUITE_KERNEL(route)(lc3s_protect_in q, int32_t* __restrict__ next_roc)
{
    const long long r = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x;
    if (r < q.n_routes) lc3s_route_out(&q, (int)r, next_roc);
}

/* the workspace's arrays of an unprotect call (lc3_srtp_shim.h) */
struct lc3s_work { unsigned long long* top1; unsigned long long* bits; long long* accepted; int32_t* first; int32_t* src; };

/* one source per lane: nothing accepted, no first item; the first lanes zero the stats */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) SUITE_KERNEL(init)(lc3s_work w, int n_ssrc, int32_t* __restrict__ stats)
{
    const long long s = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x;
    if (stats && s < LC3S_STATS_WORDS) stats[s] = 0;
    if (s < n_ssrc) { w.top1[s] = 0; w.bits[s] = 0; w.first[s] = 0x7FFFFFFF; }
}

/* One item per lane, grid-stride: checks 1 and 2.  Leaves the item's source, or -1 - its status, and for a source that has not started the smallest list index
 * among its items (a vector atomic minimum) */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) SUITE_KERNEL(scan)(lc3srtp_unprotect_call q, lc3s_work w)
{
    const long long stride = (long long)gridDim.x * LC3S_THREADS;
    for (long long i = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x; i < q.n_items; i += stride) {
        const lc3s_item it = lc3s_check((const uint8_t*)q.ring, q.ring_capacity, q.dg_offsets[i], q.dg_sizes[i], SUITE_TAG(q), q.ssrc_key, q.n_ssrc);
        w.src[i] = it.status == LC3S_OK ? it.src : -1 - (int32_t)it.status;
        if (it.status == LC3S_OK && !(q.state_in[(size_t)it.src * LC3S_STATE_WORDS + LC3S_FLAGS] & LC3S_STARTED)) atomicMin(&w.first[it.src], (int32_t)i);
    }
}

/* One item per lane, grid-stride: checks 3 to 6 against state_in, the authentication, the decryption in place; sizes_out, status, index; the source's largest
 * accepted index by a 64-bit vector atomic maximum.  stats: every lane adds to its workgroup's tally in LDS, the workgroup adds its sums with one vector atomic
 * per status at its end (as the parse does) */
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) SUITE_KERNEL(auth)(lc3srtp_unprotect_call q, lc3s_work w)
{
    SUITE_LDS
    __shared__ int tally[LC3S_STATUSES];
    if (threadIdx.x < LC3S_STATUSES) tally[threadIdx.x] = 0;
    SUITE_TABLES();
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
            const lc3s_item it = lc3s_check(ring, q.ring_capacity, off, size, SUITE_TAG(q), q.ssrc_key + s, 1);      /* the header again; the source is known */
            const int32_t* state = q.state_in + (size_t)s * LC3S_STATE_WORDS;
            const uint32_t* ctx = (const uint32_t*)q.ctx + (size_t)s * SUITE_CTX_WORDS;
            uint32_t s_l_first = 0;
            if (!(state[LC3S_FLAGS] & LC3S_STARTED)) s_l_first = lc3s_seq_at(ring, q.dg_offsets[w.first[s]]);
            lc3s_item me = it;
            me.src = s;
            SUITE_LANE(ctx);
            st = SUITE_UNPROTECT(ring, off, size, &me, state, s_l_first, ctx, &index);
            if (st == LC3S_OK) {
                size_out = size - SUITE_TAG(q); accepted = index;
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
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) SUITE_KERNEL(window)(lc3srtp_unprotect_call q, lc3s_work w)
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
extern "C" __global__ void __launch_bounds__(LC3S_THREADS) SUITE_KERNEL(state)(lc3srtp_unprotect_call q, lc3s_work w)
{
    const long long s = (long long)blockIdx.x * LC3S_THREADS + threadIdx.x;
    if (s < q.n_ssrc) lc3s_state_out(q.state_in + (size_t)s * LC3S_STATE_WORDS, q.state_out + (size_t)s * LC3S_STATE_WORDS, w.top1[s], w.bits[s]);
}

/* ---- host ---- */
#include "lc3_sibling.h"
#define SUITE_ROW(kernel) SIB_KERNEL(kernel)                        /* the name expanded before SIB_KERNEL spells it */
static const sib_kernel k_table[] = {SUITE_ROW(SUITE_KERNEL(protect)), SUITE_ROW(SUITE_KERNEL(route)), SUITE_ROW(SUITE_KERNEL(init)), SUITE_ROW(SUITE_KERNEL(scan)),
                                     SUITE_ROW(SUITE_KERNEL(auth)), SUITE_ROW(SUITE_KERNEL(window)), SUITE_ROW(SUITE_KERNEL(state))};
extern "C" long long SUITE_ABI(launch_count)(const char* kernel) { return sib_launch_count(k_table, kernel); }

extern "C" int SUITE_ABI(protect_run)(const lc3srtp_protect_call* q)
{
    if (!q || q->max_packets <= 0 || q->max_packets >= LC3S_MAX_ITEMS || !q->n_packets || q->in.n_routes <= 0 || !SUITE_TAG_OK(q->in.tag_len)) return 1;
    if (!q->in.route || !q->in.offset || !q->in.size || !q->in.status || !q->in.wire || !q->in.ctx || !q->in.roc || !q->in.seq_base || !q->in.dst) return 1;
    if (!q->out_offset || !q->out_size || !q->out_status || (q->next_roc && !q->in.next_seq)) return 1;
    if (q->in.dst_stride <= 0 || q->in.dst_stride > LC3S_MAX_STRIDE || q->in.dst_capacity < 0 || q->in.wire_capacity < 0) return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    const unsigned blocks = sib_blocks_for(q->max_packets, LC3S_THREADS, 1 << 16);
    SIB_LAUNCH(SUITE_KERNEL(protect), dim3(blocks), dim3(LC3S_THREADS), 0, s, q->in, q->max_packets, q->n_packets, q->out_offset, q->out_size, q->out_status);
    if (q->next_roc) {
        SIB_LAUNCH(SUITE_KERNEL(route), dim3(sib_blocks_for(q->in.n_routes, LC3S_THREADS, 1LL << 30)), dim3(LC3S_THREADS), 0, s, q->in, q->next_roc);
    }
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int SUITE_ABI(unprotect_run)(const lc3srtp_unprotect_call* q)
{
    if (!q || q->n_items <= 0 || q->n_items >= LC3S_MAX_ITEMS || q->n_ssrc <= 0 || q->ring_capacity < 0 || !SUITE_TAG_OK(q->tag_len)) return 1;
    if (!q->ring || !q->dg_offsets || !q->dg_sizes || !q->ssrc_key || !q->ctx || !q->state_in || !q->state_out || !q->sizes_out || !q->workspace) return 1;
    if (q->workspace_bytes < lc3s_workspace_bytes(q->n_items, q->n_ssrc)) return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    /* the workspace's arrays (lc3_srtp_shim.h) */
    lc3s_work w;
    w.top1 = (unsigned long long*)(((uintptr_t)q->workspace + 15) & ~(uintptr_t)15);
    w.bits = w.top1 + q->n_ssrc;
    w.accepted = (long long*)(w.bits + q->n_ssrc);
    w.first = (int32_t*)(w.accepted + q->n_items);
    w.src = w.first + q->n_ssrc;
    const long long per_source = q->n_ssrc > LC3S_STATS_WORDS ? q->n_ssrc : LC3S_STATS_WORDS;
    SIB_LAUNCH(SUITE_KERNEL(init), dim3(sib_blocks_for(per_source, LC3S_THREADS, 1LL << 30)), dim3(LC3S_THREADS), 0, s, w, q->n_ssrc, q->stats);
    const unsigned blocks = sib_blocks_for(q->n_items, LC3S_THREADS, 1 << 16);
    SIB_LAUNCH(SUITE_KERNEL(scan), dim3(blocks), dim3(LC3S_THREADS), 0, s, *q, w);
    SIB_LAUNCH(SUITE_KERNEL(auth), dim3(blocks), dim3(LC3S_THREADS), 0, s, *q, w);
    SIB_LAUNCH(SUITE_KERNEL(window), dim3(blocks), dim3(LC3S_THREADS), 0, s, *q, w);
    SIB_LAUNCH(SUITE_KERNEL(state), dim3(sib_blocks_for(q->n_ssrc, LC3S_THREADS, 1LL << 30)), dim3(LC3S_THREADS), 0, s, *q, w);
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}
