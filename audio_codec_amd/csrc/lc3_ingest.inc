/* lc3_ingest.inc -- the packet-ingest kernels (included by lc3_ingest.hip): a flat packet list in arrival order -> the [stream][frame] tables of decode_packed,
 * by the rule of include/lc3plus_batch.h "Packet ingest" (lc3_ingest_shim.h holds its text, shared with lc3plus_plan_ingest on the host).
 *
 * cell_item is the workspace as well as an output, which is what keeps the call free of allocations: the fill kernel sets every cell to all ones, the item
 * kernel sorts the candidates in with one atomicMin per candidate on the key rank << 29 | item - the smallest (rank, item) wins whatever order the lanes run
 * in - and the stream kernel replaces each key by its item, or -1.  LATE and EARLY are counted in their words of stats, zeroed by the fill kernel.  The status
 * kernel classes each item once more and compares it with its cell's winner.  No LDS, no scratch; plain loads and stores, integer atomics on global memory. */

/* cell_item [n_cells] all ones; stats [n_stat_words] zero (NULL: none) */
extern "C" __global__ void __launch_bounds__(256) lc3_ingest_fill_kernel(uint32_t* __restrict__ cell_key, long long n_cells, int32_t* __restrict__ stats, long long n_stat_words)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += step) cell_key[i] = LC3I_NO_KEY;
    if (stats)
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_stat_words; i += step) stats[i] = 0;
}

/* one item per lane, grid-stride: of a probe record only the status word of each channel is read */
extern "C" __global__ void __launch_bounds__(256) lc3_ingest_item_kernel(const int32_t* __restrict__ stream, const int32_t* __restrict__ seq, const int32_t* __restrict__ num_bytes,
                                                              const int32_t* __restrict__ info, const int32_t* __restrict__ base, long long n_items, int n_streams,
                                                              int channels, int seq_bits, int n_frames, uint32_t* cell_key, int32_t* stats)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += step) {
        const int s = stream[i];
        int t = 0, rank = 0;
        const int cls = lc3i_item(s, seq[i], num_bytes[i], info ? info + (size_t)i * channels * LC3I_INFO_WORDS : nullptr, channels, n_streams, base, seq_bits,
                                  n_frames, &t, &rank);
        if (cls == 0) atomicMin(cell_key + (size_t)s * n_frames + t, lc3i_key(rank, i));
        else if (stats && (cls == LC3I_LATE || cls == LC3I_EARLY)) atomicAdd(stats + (size_t)s * LC3I_STATS_WORDS + (cls == LC3I_LATE ? LC3I_ST_LATE : LC3I_ST_EARLY), 1);
    }
}

/* one stream per wave, the lanes walk its frames in steps of 64: keys -> the three tables, then the stream's count, next base and stats */
extern "C" __global__ void __launch_bounds__(256) lc3_ingest_stream_kernel(const long long* __restrict__ offsets, const int32_t* __restrict__ num_bytes, const int32_t* __restrict__ base,
                                                                const int32_t* __restrict__ floor, int n_streams, int seq_bits, int n_frames,
                                                                long long* __restrict__ out_offsets, int32_t* __restrict__ out_num_bytes, int32_t* cell_item,
                                                                int32_t* __restrict__ counts, int32_t* __restrict__ next_base, int32_t* __restrict__ stats)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long s = (long long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;           /* the same in every lane of a wave */
    if (s >= n_streams) return;
    int top = -1, won = 0;
    for (int t0 = 0; t0 < n_frames; t0 += WAVE) {
        const int t = t0 + lane;
        if (t < n_frames) {
            const size_t c = (size_t)s * n_frames + t;
            const uint32_t key = (uint32_t)cell_item[c];
            long long off = 0; int nb = 0, w = -1;
            if (key != LC3I_NO_KEY) { w = (int)(key & LC3I_ITEM_MASK); off = offsets[w]; nb = num_bytes[w]; top = t; won++; }
            out_offsets[c] = off; out_num_bytes[c] = nb; cell_item[c] = w;
        }
    }
    for (int m = WAVE / 2; m > 0; m >>= 1) {
        const int o = __shfl_xor(top, m, WAVE);
        top = o > top ? o : top;
        won += __shfl_xor(won, m, WAVE);
    }
    if (lane == 0) {
        const int count = lc3i_count(floor ? floor[s] : 0, n_frames, top);
        counts[s] = count;
        if (next_base) next_base[s] = lc3i_next_base(base[s], count, seq_bits);
        if (stats) { stats[s * LC3I_STATS_WORDS + LC3I_ST_COUNT] = count; stats[s * LC3I_STATS_WORDS + LC3I_ST_GAPS] = count - won; }   /* every winner lies below count */
    }
}

/* one item per lane, behind the stream kernel: cell_item holds the winners */
extern "C" __global__ void __launch_bounds__(256) lc3_ingest_status_kernel(const int32_t* __restrict__ stream, const int32_t* __restrict__ seq, const int32_t* __restrict__ num_bytes,
                                                                const int32_t* __restrict__ info, const int32_t* __restrict__ base, long long n_items, int n_streams,
                                                                int channels, int seq_bits, int n_frames, const int32_t* __restrict__ cell_item,
                                                                uint8_t* __restrict__ item_status)
{
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += step) {
        const int s = stream[i];
        int t = 0, rank = 0;
        int st = lc3i_item(s, seq[i], num_bytes[i], info ? info + (size_t)i * channels * LC3I_INFO_WORDS : nullptr, channels, n_streams, base, seq_bits, n_frames,
                           &t, &rank);
        if (st == 0) st = lc3i_candidate_status(rank, i, cell_item[(size_t)s * n_frames + t]);
        item_status[i] = (uint8_t)st;
    }
}
