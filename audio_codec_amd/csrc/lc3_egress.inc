/* lc3_egress.inc -- the packet-egress kernels (included by lc3_egress.hip): the [stream][frame] tables of encode_packed or of the ingest -> a compacted packet
 * list per route and, in wire mode, the frames copied behind their header rooms, by the rule of include/lc3plus_batch.h "Packet egress" (lc3_egress_shim.h
 * holds its text, shared with lc3plus_plan_egress on the host).
 *
 * A compaction with two running sums, the packet index and the byte offset, over the cells in list order, as a chain of kernels over the caller's workspace
 * (layout: lc3_egress_shim.h): classify writes one word per cell; sums reduces each tile of LC3E_TILE cells; base, one workgroup, turns the tiles' sums into
 * their bases and writes the totals; scatter scans each tile once more from its base and writes the list.  No workgroup waits for another: the kernel
 * boundaries are the only ordering.  The route kernel tallies each route's cells; the copy kernel, the only one that moves frame bytes, runs in wire mode alone. */

/* exclusive scan of (cnt, bytes) over the workgroup by wave-level scans and one exchange of the waves' sums; the workgroup's sums in *all_cnt, *all_bytes.
 * sh_c, sh_b: LC3E_THREADS / WAVE entries each */
__device__ __forceinline__ void lc3e_block_scan(int* cnt, long long* bytes, int* all_cnt, long long* all_bytes, int* sh_c, long long* sh_b)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, waves = blockDim.x / WAVE;
    int c = *cnt; long long b = *bytes;
    for (int d = 1; d < WAVE; d <<= 1) {
        const int oc = __shfl_up(c, d, WAVE);
        const long long ob = __shfl_up(b, d, WAVE);
        if (lane >= d) { c += oc; b += ob; }
    }
    __syncthreads();                                                  /* the previous use of sh_c, sh_b is over */
    if (lane == WAVE - 1) { sh_c[wave] = c; sh_b[wave] = b; }
    __syncthreads();
    int pc = 0, tc = 0; long long pb = 0, tb = 0;
    for (int w = 0; w < waves; w++) { const int wc = sh_c[w]; const long long wb = sh_b[w]; if (w < wave) { pc += wc; pb += wb; } tc += wc; tb += wb; }
    *cnt = pc + c - *cnt; *bytes = pb + b - *bytes;
    *all_cnt = tc; *all_bytes = tb;
}

/* one cell per lane: word[i] for cell i of the list order */
extern "C" __global__ void __launch_bounds__(LC3E_THREADS) lc3_egress_classify_kernel(long long n_cells, int n_streams, int n_routes, int n_frames, int order,
                                                                             const int32_t* __restrict__ route_src, const int32_t* __restrict__ counts,
                                                                             const long long* __restrict__ offsets, const int32_t* __restrict__ num_bytes,
                                                                             const uint8_t* __restrict__ flags, int max_frame_bytes, long long capacity, int skip_mask,
                                                                             int32_t* __restrict__ word)
{
    const long long i = (long long)blockIdx.x * LC3E_THREADS + threadIdx.x;
    if (i >= n_cells) return;
    int r, t;
    lc3e_cell_rt(i, n_routes, n_frames, order, &r, &t);
    word[i] = lc3e_cell_word(r, t, n_streams, route_src, counts, n_frames, offsets, num_bytes, flags, max_frame_bytes, capacity, skip_mask);
}

/* one tile per workgroup: sums[tile] = {SENT cells, their advance in bytes} */
extern "C" __global__ void __launch_bounds__(LC3E_THREADS) lc3_egress_sums_kernel(const int32_t* __restrict__ word, long long n_cells, int wire_mode, int header_room, int align,
                                                                         long long* __restrict__ sums)
{
    __shared__ int sh_c[LC3E_THREADS / WAVE];
    __shared__ long long sh_b[LC3E_THREADS / WAVE];
    const long long j0 = (long long)blockIdx.x * LC3E_TILE + (long long)threadIdx.x * LC3E_ITEMS;
    int cnt = 0; long long bytes = 0;
    for (int k = 0; k < LC3E_ITEMS; k++)
        if (j0 + k < n_cells) { const int32_t w = word[j0 + k]; cnt += w > 0; bytes += lc3e_advance(w, wire_mode, header_room, align); }
    int ac; long long ab;
    lc3e_block_scan(&cnt, &bytes, &ac, &ab, sh_c, sh_b);
    if (threadIdx.x == 0) { sums[2 * (long long)blockIdx.x] = ac; sums[2 * (long long)blockIdx.x + 1] = ab; }
}

/* one workgroup: the tiles' sums -> the tiles' bases, in place, and the call's totals */
extern "C" __global__ void __launch_bounds__(LC3E_THREADS) lc3_egress_base_kernel(long long* __restrict__ sums, long long n_tiles, long long* __restrict__ n_packets,
                                                                         long long* __restrict__ wire_total)
{
    __shared__ int sh_c[LC3E_THREADS / WAVE];
    __shared__ long long sh_b[LC3E_THREADS / WAVE];
    long long run_c = 0, run_b = 0;
    for (long long b0 = 0; b0 < n_tiles; b0 += LC3E_THREADS) {
        const long long b = b0 + threadIdx.x;
        int cnt = b < n_tiles ? (int)sums[2 * b] : 0;                 /* a tile holds at most LC3E_TILE packets, LC3E_THREADS tiles fit an int */
        long long bytes = b < n_tiles ? sums[2 * b + 1] : 0;
        int ac; long long ab;
        lc3e_block_scan(&cnt, &bytes, &ac, &ab, sh_c, sh_b);
        if (b < n_tiles) { sums[2 * b] = run_c + cnt; sums[2 * b + 1] = run_b + bytes; }
        run_c += ac; run_b += ab;
    }
    if (threadIdx.x == 0) { *n_packets = run_c; if (wire_total) *wire_total = run_b; }
}

/* one tile per workgroup, behind the base kernel: every SENT cell's list entry, every cell's status */
extern "C" __global__ void __launch_bounds__(LC3E_THREADS) lc3_egress_scatter_kernel(const int32_t* __restrict__ word, long long n_cells, const long long* __restrict__ base,
                                                                            int n_routes, int n_frames, int order, const int32_t* __restrict__ route_src,
                                                                            const int32_t* __restrict__ seq_base, int seq_bits, const long long* __restrict__ offsets,
                                                                            int wire_mode, int header_room, int align, long long wire_capacity, lc3e_list L)
{
    __shared__ int sh_c[LC3E_THREADS / WAVE];
    __shared__ long long sh_b[LC3E_THREADS / WAVE];
    const long long j0 = (long long)blockIdx.x * LC3E_TILE + (long long)threadIdx.x * LC3E_ITEMS;
    int32_t w[LC3E_ITEMS];
    int cnt = 0; long long bytes = 0;
#pragma unroll
    for (int k = 0; k < LC3E_ITEMS; k++) {
        w[k] = j0 + k < n_cells ? word[j0 + k] : 0;
        cnt += w[k] > 0; bytes += lc3e_advance(w[k], wire_mode, header_room, align);
    }
    int ac; long long ab;
    lc3e_block_scan(&cnt, &bytes, &ac, &ab, sh_c, sh_b);
    long long p = base[2 * (long long)blockIdx.x] + cnt, run = base[2 * (long long)blockIdx.x + 1] + bytes;
#pragma unroll
    for (int k = 0; k < LC3E_ITEMS; k++) {
        if (j0 + k >= n_cells) break;
        int r, t;
        lc3e_cell_rt(j0 + k, n_routes, n_frames, order, &r, &t);
        int st = -w[k];
        if (w[k] > 0) {
            st = lc3e_emit(&L, p, r, t, route_src ? route_src[r] : r, w[k], run, seq_base, seq_bits, n_frames, offsets, wire_mode, header_room, wire_capacity);
            p++; run += lc3e_advance(w[k], wire_mode, header_room, align);
        }
        if (L.status) L.status[(size_t)r * n_frames + t] = (uint8_t)st;
    }
}

/* one route per wave, behind the scatter kernel: the lanes walk the route's cells in front of its count in steps of 64 (status: by (route, frame), NULL
 * without stats) */
extern "C" __global__ void __launch_bounds__(LC3E_THREADS) lc3_egress_route_kernel(int n_streams, int n_routes, int n_frames, const int32_t* __restrict__ route_src,
                                                                          const int32_t* __restrict__ counts, const int32_t* __restrict__ seq_base, int seq_bits,
                                                                          const uint8_t* __restrict__ status, int32_t* __restrict__ next_seq, int32_t* __restrict__ stats)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long r = (long long)blockIdx.x * (LC3E_THREADS / WAVE) + threadIdx.x / WAVE;          /* the same in every lane of a wave */
    if (r >= n_routes) return;
    int s = 0;
    const int c = lc3e_route(route_src, (int)r, n_streams, counts, n_frames, &s);
    int sent = 0, holes = 0, over = 0;
    if (stats)
        for (int t = lane; t < c; t += WAVE) {
            const int st = status[(size_t)r * n_frames + t];
            sent += (st & LC3E_SENT) != 0; over += (st & LC3E_OVERFLOW) != 0; holes += (st & (LC3E_LOST | LC3E_INVALID | LC3E_SKIPPED)) != 0;
        }
    for (int m = WAVE / 2; m > 0; m >>= 1) { sent += __shfl_xor(sent, m, WAVE); holes += __shfl_xor(holes, m, WAVE); over += __shfl_xor(over, m, WAVE); }
    if (lane == 0) lc3e_route_out((int)r, c, sent, holes, over, seq_base, seq_bits, next_seq, stats);
}

/* The copy kernel: LC3E_COPY_LANES lanes per packet, so LC3E_THREADS / LC3E_COPY_LANES packets per workgroup; packets behind *n_packets and packets that do not
 * fit the wire buffer are left alone.  A frame lies at any byte address and goes to any byte address in the runs of lc3e_copy_layout.  Its 16-byte pieces are
 * stored whole, each from the four or five aligned source words that hold its bytes, realigned in registers by a funnel shift of neighbouring words; the head
 * and tail words likewise from one or two source words, and the at most three head and three tail bytes each out of its aligned source word.  The small runs
 * are spread over the lanes - lanes 0 .. 2 the head's, lanes 3 .. 5 the tail's - so that all head and tail bytes go in one store instruction and all head and
 * tail words in another.  No word is read that holds no byte of the frame, no byte is written outside the frame's place. */
#define LC3E_COPY_LANES 8
__device__ __forceinline__ uint32_t lc3e_src_word(uintptr_t a) { return *(const uint32_t*)a; }
/* the four bytes at byte address s, all of them the frame's */
__device__ __forceinline__ uint32_t lc3e_src_dword(uintptr_t s)
{
    const uintptr_t a = s & ~(uintptr_t)3;
    const int sh = (int)(s & 3) * 8;
    const uint32_t w0 = lc3e_src_word(a);
    return sh ? __funnelshift_r(w0, lc3e_src_word(a + 4), sh) : w0;
}
extern "C" __global__ void __launch_bounds__(LC3E_THREADS) lc3_egress_copy_kernel(const uint8_t* __restrict__ frames, long long capacity, const long long* __restrict__ n_packets,
                                                                         const long long* __restrict__ pkt_from, const long long* __restrict__ pkt_offset,
                                                                         const int32_t* __restrict__ pkt_size, int header_room, uint8_t* __restrict__ wire,
                                                                         long long wire_capacity)
{
    const int l = threadIdx.x & (LC3E_COPY_LANES - 1);
    const long long p = (long long)blockIdx.x * (LC3E_THREADS / LC3E_COPY_LANES) + threadIdx.x / LC3E_COPY_LANES;
    if (p >= *n_packets) return;
    const int32_t size = pkt_size[p];
    const long long at = pkt_offset[p], from = pkt_from[p];
    const int n = size - header_room;
    if (n <= 0 || at < 0 || !lc3e_fits(at, size, 1, wire_capacity)) return;
    if (from < 0 || from > capacity - n) return;                      /* the classify kernel has said so already */
    const uintptr_t src = (uintptr_t)frames + (uintptr_t)from, dst = (uintptr_t)wire + (uintptr_t)at + (uintptr_t)header_room;
    const lc3e_copy_plan c = lc3e_copy_layout(dst, n);
    const int body = c.hb + 4 * c.hd, tail = body + 16 * c.pieces;   /* where the pieces and the tail words start in the frame */
    /* head and tail bytes: one load and one store for both */
    const int bi = l < 3 ? (l < c.hb ? l : -1) : l < 6 ? (l - 3 < c.tb ? tail + 4 * c.td + l - 3 : -1) : -1;
    if (bi >= 0) { const uintptr_t a = src + bi; *(uint8_t*)(dst + bi) = (uint8_t)(lc3e_src_word(a & ~(uintptr_t)3) >> ((a & 3) * 8)); }
    /* head and tail words */
    const int di = l < 3 ? (l < c.hd ? c.hb + 4 * l : -1) : l < 6 ? (l - 3 < c.td ? tail + 4 * (l - 3) : -1) : -1;
    if (di >= 0) *(uint32_t*)(dst + di) = lc3e_src_dword(src + di);
    const uintptr_t s0 = src + body, d0 = dst + body;                 /* d0 is 16-byte aligned wherever pieces > 0 */
    const int sh = (int)(s0 & 3) * 8;
    for (int k = l; k < c.pieces; k += LC3E_COPY_LANES) {
        const uintptr_t a = (s0 + 16 * (uintptr_t)k) & ~(uintptr_t)3;
        const uint32_t w0 = lc3e_src_word(a), w1 = lc3e_src_word(a + 4), w2 = lc3e_src_word(a + 8), w3 = lc3e_src_word(a + 12);
        uint4 v = make_uint4(w0, w1, w2, w3);
        if (sh) {                                                     /* the fifth word holds the piece's last byte exactly where sh != 0 */
            const uint32_t w4 = lc3e_src_word(a + 16);
            v = make_uint4(__funnelshift_r(w0, w1, sh), __funnelshift_r(w1, w2, sh), __funnelshift_r(w2, w3, sh), __funnelshift_r(w3, w4, sh));
        }
        *(uint4*)(d0 + 16 * (uintptr_t)k) = v;
    }
}
