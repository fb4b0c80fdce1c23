/* lc3_red.inc -- the redundant-audio kernels (included by lc3_red.hip): the egress's frame tables and in-place packet list -> RFC 2198 packets in a wire buffer,
 * and the parse's items -> one item per block, by the rules of include/lc3plus_batch.h "Redundant audio" (lc3_red_shim.h holds their text, shared with
 * lc3plus_plan_red_pack and lc3plus_plan_red_unpack on the host).  Every offset into the frames, the ring and the wire buffer is 64 bits wide.
 *
 * The pack is the egress's chain once more (lc3_egress.inc), over list entries instead of cells: size writes one word and one mask per packet into the caller's
 * workspace; sums reduces each tile of LC3RED_TILE packets; base, one workgroup, turns the tiles' sums into their bases and writes the total; scatter scans each
 * tile once more from its base and writes the packet records; copy, the only kernel that moves payload bytes, writes the headers and copies the blocks; tail
 * hands the last frames of every stream to the next call.  No workgroup waits for another: the kernel boundaries are the only ordering. */

/* exclusive scan of bytes over the workgroup by wave-level scans and one exchange of the waves' sums; the workgroup's sum in *all.  sh: LC3RED_THREADS / WAVE entries */
__device__ __forceinline__ void lc3red_block_scan(long long* bytes, long long* all, long long* sh)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, waves = blockDim.x / WAVE;
    long long b = *bytes;
    for (int d = 1; d < WAVE; d <<= 1) {
        const long long ob = __shfl_up(b, d, WAVE);
        if (lane >= d) b += ob;
    }
    __syncthreads();                                                  /* the previous use of sh is over */
    if (lane == WAVE - 1) sh[wave] = b;
    __syncthreads();
    long long pb = 0, tb = 0;
    for (int w = 0; w < waves; w++) { const long long wb = sh[w]; if (w < wave) pb += wb; tb += wb; }
    *bytes = pb + b - *bytes;
    *all = tb;
}

/* one packet per lane: size[p] and mask[p] for every list entry in front of *n_packets.  The first lanes of the grid zero route_stats for the copy kernel */
extern "C" __global__ void __launch_bounds__(LC3RED_THREADS) lc3_red_size_kernel(lc3red_pack_in q, long long max_packets, const long long* __restrict__ n_packets,
                                                                         int32_t* __restrict__ size, uint8_t* __restrict__ mask, int32_t* __restrict__ route_stats)
{
    const long long p = (long long)blockIdx.x * LC3RED_THREADS + threadIdx.x;
    if (route_stats)
        for (long long k = p; k < (long long)q.n_routes * LC3RED_RS_WORDS; k += (long long)gridDim.x * LC3RED_THREADS) route_stats[k] = 0;
    if (p >= lc3red_count(n_packets, max_packets)) return;
    int s = 0, m = 0;
    size[p] = lc3red_packet(&q, q.pkt_route[p], q.pkt_frame[p], &s, &m);
    mask[p] = (uint8_t)m;
}

/* one tile per workgroup: sums[tile] = the advance of its packets in bytes */
extern "C" __global__ void __launch_bounds__(LC3RED_THREADS) lc3_red_sums_kernel(const int32_t* __restrict__ size, long long max_packets, const long long* __restrict__ n_packets,
                                                                         int align, long long* __restrict__ sums)
{
    __shared__ long long sh[LC3RED_THREADS / WAVE];
    const long long n = lc3red_count(n_packets, max_packets);
    const long long j0 = (long long)blockIdx.x * LC3RED_TILE + (long long)threadIdx.x * LC3RED_ITEMS;
    long long bytes = 0, all;
    for (int k = 0; k < LC3RED_ITEMS; k++)
        if (j0 + k < n) bytes += lc3red_advance(size[j0 + k], align);
    lc3red_block_scan(&bytes, &all, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

/* one workgroup: the tiles' sums -> the tiles' bases, in place, and the call's total */
extern "C" __global__ void __launch_bounds__(LC3RED_THREADS) lc3_red_base_kernel(long long* __restrict__ sums, long long n_tiles, long long* __restrict__ wire_total)
{
    __shared__ long long sh[LC3RED_THREADS / WAVE];
    long long run = 0;
    for (long long b0 = 0; b0 < n_tiles; b0 += LC3RED_THREADS) {
        const long long b = b0 + threadIdx.x;
        long long bytes = b < n_tiles ? sums[b] : 0, all;
        lc3red_block_scan(&bytes, &all, sh);
        if (b < n_tiles) sums[b] = run + bytes;
        run += all;
    }
    if (threadIdx.x == 0 && wire_total) *wire_total = run;
}

/* one tile per workgroup, behind the base kernel: every packet's record */
extern "C" __global__ void __launch_bounds__(LC3RED_THREADS) lc3_red_scatter_kernel(const int32_t* __restrict__ size, const uint8_t* __restrict__ mask, long long max_packets,
                                                                            const long long* __restrict__ n_packets, const long long* __restrict__ base, int align,
                                                                            long long wire_capacity, long long* __restrict__ red_offset, int32_t* __restrict__ red_size,
                                                                            uint8_t* __restrict__ red_flags, uint8_t* __restrict__ red_blocks)
{
    __shared__ long long sh[LC3RED_THREADS / WAVE];
    const long long n = lc3red_count(n_packets, max_packets);
    const long long j0 = (long long)blockIdx.x * LC3RED_TILE + (long long)threadIdx.x * LC3RED_ITEMS;
    int32_t w[LC3RED_ITEMS];
    long long bytes = 0, all;
#pragma unroll
    for (int k = 0; k < LC3RED_ITEMS; k++) {
        w[k] = j0 + k < n ? size[j0 + k] : 0;
        bytes += lc3red_advance(w[k], align);
    }
    lc3red_block_scan(&bytes, &all, sh);
    long long run = base[blockIdx.x] + bytes;
#pragma unroll
    for (int k = 0; k < LC3RED_ITEMS; k++) {
        const long long p = j0 + k;
        if (p >= n) break;
        red_offset[p] = run; red_size[p] = w[k];
        if (red_flags) red_flags[p] = (uint8_t)(w[k] <= 0 ? LC3RED_PKT_BAD : lc3e_fits(run, w[k], 1, wire_capacity) ? 0 : LC3E_PKT_OVERFLOW);
        if (red_blocks) red_blocks[p] = (uint8_t)(mask[p] & 15);
        run += lc3red_advance(w[k], align);
    }
}

/* The egress's copy rule (lc3_egress.inc, lc3e_copy_layout) for one run of n bytes from byte address src to byte address dst, by the LC3RED_COPY_LANES lanes of a
 * packet, l this lane's index: 16-byte pieces stored whole, each from the four or five aligned source words that hold its bytes, realigned in registers; head
 * and tail words likewise; the at most three head and three tail bytes each out of its aligned source word.  No word is read that holds no byte of the run, no
 * byte is written outside its place. */
__device__ __forceinline__ uint32_t lc3red_src_word(uintptr_t a) { return *(const uint32_t*)a; }
__device__ __forceinline__ uint32_t lc3red_src_dword(uintptr_t s)
{
    const uintptr_t a = s & ~(uintptr_t)3;
    const int sh = (int)(s & 3) * 8;
    const uint32_t w0 = lc3red_src_word(a);
    return sh ? __funnelshift_r(w0, lc3red_src_word(a + 4), sh) : w0;
}
__device__ __forceinline__ void lc3red_copy(uintptr_t src, uintptr_t dst, int n, int l)
{
    const lc3e_copy_plan c = lc3e_copy_layout(dst, n);
    const int body = c.hb + 4 * c.hd, tail = body + 16 * c.pieces;
    const int bi = l < 3 ? (l < c.hb ? l : -1) : l < 6 ? (l - 3 < c.tb ? tail + 4 * c.td + l - 3 : -1) : -1;
    if (bi >= 0) { const uintptr_t a = src + bi; *(uint8_t*)(dst + bi) = (uint8_t)(lc3red_src_word(a & ~(uintptr_t)3) >> ((a & 3) * 8)); }
    const int di = l < 3 ? (l < c.hd ? c.hb + 4 * l : -1) : l < 6 ? (l - 3 < c.td ? tail + 4 * (l - 3) : -1) : -1;
    if (di >= 0) *(uint32_t*)(dst + di) = lc3red_src_dword(src + di);
    const uintptr_t s0 = src + body, d0 = dst + body;                 /* d0 is 16-byte aligned wherever pieces > 0 */
    const int sh = (int)(s0 & 3) * 8;
    for (int k = l; k < c.pieces; k += LC3RED_COPY_LANES) {
        const uintptr_t a = (s0 + 16 * (uintptr_t)k) & ~(uintptr_t)3;
        const uint32_t w0 = lc3red_src_word(a), w1 = lc3red_src_word(a + 4), w2 = lc3red_src_word(a + 8), w3 = lc3red_src_word(a + 12);
        uint4 v = make_uint4(w0, w1, w2, w3);
        if (sh) {                                                     /* the fifth word holds the piece's last byte exactly where sh != 0 */
            const uint32_t w4 = lc3red_src_word(a + 16);
            v = make_uint4(__funnelshift_r(w0, w1, sh), __funnelshift_r(w1, w2, sh), __funnelshift_r(w2, w3, sh), __funnelshift_r(w3, w4, sh));
        }
        *(uint4*)(d0 + 16 * (uintptr_t)k) = v;
    }
}

/* The copy kernel: LC3RED_COPY_LANES lanes per packet; packets behind *n_packets, BAD packets and packets that do not fit the wire buffer write nothing.  A
 * block's header goes out of a register, a byte per lane (lanes 0 .. 3; lane 4 the final byte), the blocks oldest first and then the primary by lc3red_copy.
 * The workgroup then adds its packets to their routes' stats, which the size kernel has zeroed. */
extern "C" __global__ void __launch_bounds__(LC3RED_THREADS) lc3_red_copy_kernel(lc3red_pack_in q, long long max_packets, const long long* __restrict__ n_packets,
                                                                         const int32_t* __restrict__ size, const uint8_t* __restrict__ mask,
                                                                         const long long* __restrict__ red_offset, uint8_t* __restrict__ wire,
                                                                         int32_t* __restrict__ route_stats)
{
    enum { PER = LC3RED_THREADS / LC3RED_COPY_LANES };
    __shared__ int32_t sh_r[PER], sh_k[PER], sh_b[PER], sh_m[PER];
    const int l = threadIdx.x & (LC3RED_COPY_LANES - 1), slot = threadIdx.x / LC3RED_COPY_LANES;
    const long long p = (long long)blockIdx.x * PER + slot;
    const int32_t sz = p < lc3red_count(n_packets, max_packets) ? size[p] : 0;
    int r = -1, k = 0, missed = 0, block_bytes = 0;
    if (sz > 0) {                                                     /* else behind the list, or BAD: the size kernel has said so, nothing of the entry is looked at again */
        const int m = mask[p] & 15, t = q.pkt_frame[p];
        r = q.pkt_route[p]; k = __popc(m); missed = mask[p] >> 4;
        const int s = q.route_src ? q.route_src[r] : r, pt = q.block_pt[r];
        const long long at = red_offset[p];
        const int fit = at >= 0 && lc3e_fits(at, sz, 1, q.wire_capacity);
        uintptr_t hdr = (uintptr_t)wire + (uintptr_t)at + (uintptr_t)q.header_room, body = hdr + 4 * k + 1, src = 0;
        for (int j = q.max_depth; j >= 1; j--) {
            if (!(m >> (j - 1) & 1)) continue;
            const int32_t bs = lc3red_block(&q, s, t - j, &src);
            block_bytes += bs;
            if (!fit) continue;
            if (l < 4) *(uint8_t*)(hdr + l) = (uint8_t)(lc3red_header(pt, j * q.ts_step, bs) >> (8 * l));
            lc3red_copy(src, body, bs, l);
            hdr += 4; body += bs;
        }
        if (fit) {
            const int32_t nb = lc3red_block(&q, s, t, &src);
            if (l == 4) *(uint8_t*)hdr = (uint8_t)(pt & 127);
            lc3red_copy(src, body, nb, l);
        }
    }
    if (!route_stats) return;                                         /* the same in every lane of the grid */
    /* the stats: neighbouring packets of one route - a whole workgroup's in a stream-major list - are added up in LDS and reach the route's words as one atomic
     * each.  (One atomic per packet and word was measured first: the adds to one route's 16 bytes go one behind the other - DESIGN 10o.) */
    if (l == 0) { sh_r[slot] = r; sh_k[slot] = k; sh_b[slot] = block_bytes; sh_m[slot] = missed; }
    __syncthreads();
    if (threadIdx.x < PER && sh_r[threadIdx.x] >= 0 && (threadIdx.x == 0 || sh_r[threadIdx.x - 1] != sh_r[threadIdx.x])) {
        const int r0 = sh_r[threadIdx.x];
        int packets = 0, blocks = 0, bytes = 0, miss = 0;
        for (int i = threadIdx.x; i < PER && sh_r[i] == r0; i++) { packets++; blocks += sh_k[i]; bytes += sh_b[i]; miss += sh_m[i]; }
        int32_t* st = route_stats + (size_t)r0 * LC3RED_RS_WORDS;
        atomicAdd(st + LC3RED_RS_PACKETS, packets);
        if (blocks) { atomicAdd(st + LC3RED_RS_BLOCKS, blocks); atomicAdd(st + LC3RED_RS_BLOCK_BYTES, bytes); }
        if (miss) atomicAdd(st + LC3RED_RS_MISSED, miss);
    }
}

/* The tail kernel: LC3RED_COPY_LANES lanes per entry (s, g) of the next call's history: its size, and its bytes into the fixed slot */
extern "C" __global__ void __launch_bounds__(LC3RED_THREADS) lc3_red_tail_kernel(lc3red_pack_in q, uint8_t* __restrict__ tail_bytes_out, int32_t* __restrict__ tail_sizes_out)
{
    const int l = threadIdx.x & (LC3RED_COPY_LANES - 1);
    const long long e = (long long)blockIdx.x * (LC3RED_THREADS / LC3RED_COPY_LANES) + threadIdx.x / LC3RED_COPY_LANES;
    if (e >= (long long)q.n_streams * q.max_depth) return;
    const int s = (int)(e / q.max_depth), g = (int)(e - (long long)s * q.max_depth);
    uintptr_t src = 0;
    const int32_t nb = lc3red_tail(&q, s, g, &src);
    if (l == 0) tail_sizes_out[e] = nb;
    if (nb > 0) lc3red_copy(src, (uintptr_t)tail_bytes_out + (uintptr_t)e * (uintptr_t)q.tail_stride, nb, l);
}

/* zeroes the unpack call's stats in front of the unpack kernel */
extern "C" __global__ void __launch_bounds__(WAVE) lc3_red_fill_kernel(int32_t* __restrict__ stats)
{
    if (threadIdx.x < LC3RED_STATS_WORDS) stats[threadIdx.x] = 0;
}

/* One item per lane, grid-stride.  Of a payload a lane reads the first byte of each header and, of the first max_red, the other three: aligned words realigned in
 * registers.  stats: the lanes tally in LDS, the workgroup adds its sums with one vector atomic per word at its end */
extern "C" __global__ void __launch_bounds__(LC3RED_THREADS) lc3_red_unpack_kernel(lc3red_unpack_io q, long long n_items, int32_t* __restrict__ stats)
{
    __shared__ int tally[LC3RED_TALLIES];
    if (threadIdx.x < LC3RED_TALLIES) tally[threadIdx.x] = 0;
    __syncthreads();
    const long long stride = (long long)gridDim.x * LC3RED_THREADS;
    for (long long i = (long long)blockIdx.x * LC3RED_THREADS + threadIdx.x; i < n_items; i += stride) {
        int drops[3] = {0, 0, 0};
        const int st = lc3red_unpack(&q, i, drops);
        if (stats) {
            atomicAdd(&tally[st], 1);
            if (drops[0]) atomicAdd(&tally[LC3RED_ST_DROP_TYPE], drops[0]);
            if (drops[1]) atomicAdd(&tally[LC3RED_ST_DROP_OFFSET], drops[1]);
            if (drops[2]) atomicAdd(&tally[LC3RED_ST_DROP_EMPTY], drops[2]);
        }
    }
    if (stats) {
        __syncthreads();
        if (threadIdx.x < LC3RED_TALLIES && tally[threadIdx.x]) atomicAdd(stats + threadIdx.x, tally[threadIdx.x]);
    }
}
