/* lc3_util_kernels.inc -- the small kernels beside the codec's own, last in the plain object of lc3_kernels.hip (which includes this file): stream lifecycle,
 * the plan and tail kernels of per-frame rates and bandwidths from device memory, the offsets of packed output, and the test hook of lc3_fastmath.h. */

/* ---- stream lifecycle: one kernel for the encoder and the decoder (include/lc3plus_batch.h: lc3plus_{enc,dec}_batch_{reset,export,import}_streams) ----
 * LC3D_SS_RESET : the listed channel-streams' state rows <- the batch's fresh-row template, and with cfg their configuration entries <- cfg [n][channels]
 * LC3D_SS_EXPORT: the listed streams' rows -> blob i (LC3D_SS_HEADER bytes of header h0..h3, then the stream's rows, channel 0 first), back to back in list order
 * LC3D_SS_IMPORT: blob i -> the rows of stream list[i] where its header equals h0..h3; status[i] = 1 and the stream untouched where it does not
 * One wave per channel row.  A row is 240 (encoder), 315 (encoder, large layout) or 614 (decoder) 16-byte chunks: four to ten dwordx4 loads and stores per
 * lane, enough to keep a wave's memory pipeline busy, and the rows of a stereo stream are independent.  A workgroup per stream would only add a barrier for
 * the header decision, which the wave of each row takes from its own lane 0.  list null: stream i (create).  Rows, template and blobs are 16-byte aligned
 * (row lengths are multiples of 4 words; the host checks a device blob's address). */
extern "C" __global__ void __launch_bounds__(WAVE) lc3_stream_state_kernel(int mode, float* __restrict__ state, int row_words, int channels, const int* __restrict__ list,
                                                                           int n, const float* __restrict__ tmpl, uint8_t* __restrict__ blob, uint32_t h0, uint32_t h1,
                                                                           uint32_t h2, uint32_t h3, uint8_t* __restrict__ status, const uint32_t* __restrict__ cfg,
                                                                           uint32_t* __restrict__ chans, int cfg_words)
{
    const int lane = threadIdx.x;
    const int i = (int)(blockIdx.x / (unsigned)channels), ch = (int)(blockIdx.x % (unsigned)channels);
    if (i >= n) return;
    const size_t cs = (size_t)(list ? list[i] : i) * channels + ch;
    float4* row = (float4*)(state + cs * row_words);
    const int n4 = row_words >> 2;
    if (mode == LC3D_SS_RESET) {
        const float4* t4 = (const float4*)tmpl;
        for (int k = lane; k < n4; k += WAVE) row[k] = t4[k];
        if (cfg) for (int k = lane; k < cfg_words; k += WAVE) chans[cs * cfg_words + k] = cfg[((size_t)i * channels + ch) * cfg_words + k];
        return;
    }
    uint8_t* b = blob + (size_t)i * (LC3D_SS_HEADER + (size_t)channels * row_words * 4);
    float4* brow = (float4*)(b + LC3D_SS_HEADER + (size_t)ch * row_words * 4);
    if (mode == LC3D_SS_EXPORT) {
        if (ch == 0 && lane == 0) *(uint4*)b = make_uint4(h0, h1, h2, h3);
        for (int k = lane; k < n4; k += WAVE) brow[k] = row[k];
        return;
    }
    int ok = 0;                                                       /* import: lane 0 reads the header and decides, the wave follows before it writes */
    if (lane == 0) { const uint4 h = *(const uint4*)b; ok = h.x == h0 && h.y == h1 && h.z == h2 && h.w == h3; }
    ok = __builtin_amdgcn_readfirstlane(ok);
    if (status && ch == 0 && lane == 0) status[i] = ok ? 0 : 1;
    if (!ok) return;
    for (int k = lane; k < n4; k += WAVE) row[k] = brow[k];
}

/* ---- per-frame rates and bandwidths from device memory (include/lc3plus_batch.h: lc3plus_enc_batch_encode_rates_device) ----
 * Plan kernel: one stream per lane walks its T frames in order - the carry is serial per stream, the frames of a stream are not - with the rule of
 * lc3d_enc_frame_step (lc3_plan.h).  It is the only reader of the caller's rates [stream][T] and bandwidths [stream][T] (either may be null) and writes
 * what the per-frame kernels take (fsz with rates, bwf with bandwidths: the bytes and the bandwidth in force of every stream-frame), the caller's
 * num_bytes and flags (null or [stream][T]), and each stream's carry after the call: into carry (for the next plan kernel) and into pend (for this call's
 * tail kernel).  seed (not null): start from the configuration on the device instead of from carry, after the host has changed it.  Where T is a
 * multiple of 4 and every array is aligned for it, a lane moves four frames per access (16 bytes of rates / bandwidths / sizes); T is a kernel argument,
 * so the loop is wave-uniform. */
extern "C" __global__ void __launch_bounds__(WAVE) lc3_enc_plan_rates_kernel(lc3d_rate_rule r, const int32_t* __restrict__ rates, const int32_t* __restrict__ bws,
                                                                             int T, int n_streams, int4* __restrict__ carry, const lc3d_chan* __restrict__ seed,
                                                                             uint16_t* __restrict__ fsz, uint16_t* __restrict__ bwf, int32_t* __restrict__ num_bytes,
                                                                             uint8_t* __restrict__ flags, int4* __restrict__ pend, int vec4)
{
    const int s = (int)(blockIdx.x * WAVE + threadIdx.x);
    if (s >= n_streams) return;
    int rate, bytes, bw;
    if (seed) {
        const lc3d_chan* ch = seed + (size_t)s * r.channels;
        rate = ch[0].bitrate; bw = ch[0].bandwidth; bytes = ch[0].nbytes;
        if (r.channels > 1) bytes += ch[1].nbytes;
    } else { const int4 c = carry[s]; rate = c.x; bytes = c.y; bw = c.z; }
    const size_t row = (size_t)s * T;
    if (vec4) {
        for (int t = 0; t < T; t += 4) {
            const size_t i = row + t;
            const int4 rv = rates ? *(const int4*)(rates + i) : make_int4(0, 0, 0, 0);
            const int4 bv = bws ? *(const int4*)(bws + i) : make_int4(0, 0, 0, 0);
            int f0, f1, f2, f3; int z0, z1, z2, z3; int w0, w1, w2, w3;
            f0 = lc3d_enc_frame_step(&r, rates != nullptr, rv.x, bws != nullptr, bv.x, &rate, &bytes, &bw); z0 = bytes; w0 = bw;
            f1 = lc3d_enc_frame_step(&r, rates != nullptr, rv.y, bws != nullptr, bv.y, &rate, &bytes, &bw); z1 = bytes; w1 = bw;
            f2 = lc3d_enc_frame_step(&r, rates != nullptr, rv.z, bws != nullptr, bv.z, &rate, &bytes, &bw); z2 = bytes; w2 = bw;
            f3 = lc3d_enc_frame_step(&r, rates != nullptr, rv.w, bws != nullptr, bv.w, &rate, &bytes, &bw); z3 = bytes; w3 = bw;
            if (rates) *(uint2*)(fsz + i) = make_uint2((unsigned)z0 | (unsigned)z1 << 16, (unsigned)z2 | (unsigned)z3 << 16);
            if (bws) *(uint2*)(bwf + i) = make_uint2((unsigned)w0 | (unsigned)w1 << 16, (unsigned)w2 | (unsigned)w3 << 16);
            if (num_bytes) *(int4*)(num_bytes + i) = make_int4(z0, z1, z2, z3);
            if (flags) *(unsigned*)(flags + i) = (unsigned)f0 | (unsigned)f1 << 8 | (unsigned)f2 << 16 | (unsigned)f3 << 24;
        }
    } else {
        for (int t = 0; t < T; t++) {
            const size_t i = row + t;
            const int f = lc3d_enc_frame_step(&r, rates != nullptr, rates ? rates[i] : 0, bws != nullptr, bws ? bws[i] : 0, &rate, &bytes, &bw);
            if (rates) fsz[i] = (uint16_t)bytes;
            if (bws) bwf[i] = (uint16_t)bw;
            if (num_bytes) num_bytes[i] = bytes;
            if (flags) flags[i] = (uint8_t)f;
        }
    }
    const int4 e = make_int4(rate, bytes, bw, 0);
    carry[s] = e; pend[s] = e;
}
/* Packed output (lc3plus_enc_batch_encode_packed): the offsets of the call's frames, an exclusive scan of their sizes in the caller's order (stream-major:
 * j = s T + t, frame-major: j = t S + s) with 64-bit sums, as a reduce / scan / add chain of three kernels over tiles of PKS_TILE frames.  A frame's size
 * is fsz[s][t] (per-frame rates: the plan kernel's sizes), else pend[s].y (bandwidths alone: the stream's bytes the plan kernel carried), else the sum of
 * the stream's channel bytes in chans. */
__device__ __forceinline__ int pks_size(const PkSrc& q, long long j, size_t* idx)
{
    int s, t;
    if (q.order) { t = (int)(j / q.S); s = (int)(j - (long long)t * q.S); } else { s = (int)(j / q.T); t = (int)(j - (long long)s * q.T); }
    *idx = (size_t)s * q.T + t;
    if (q.fsz) return q.fsz[*idx];
    if (q.pend) return q.pend[s].y;
    int nb = 0;
    for (int c = 0; c < q.channels; c++) nb += q.chans[(size_t)s * q.channels + c].nbytes;
    return nb;
}
/* exclusive scan of one value per thread over the workgroup; returns the workgroup's sum in *all */
__device__ __forceinline__ long long pks_block_scan(long long v, long long* sh, long long* all)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < PKS_THREADS; d <<= 1) {
        const long long a = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += a;
        __syncthreads();
    }
    const long long inc = sh[tid];
    *all = sh[PKS_THREADS - 1];
    __syncthreads();
    return inc - v;
}
extern "C" __global__ void __launch_bounds__(PKS_THREADS) lc3_pack_sums_kernel(PkSrc q, long long n, long long* __restrict__ bsum)
{
    __shared__ long long sh[PKS_THREADS];
    const long long j0 = (long long)blockIdx.x * PKS_TILE + (long long)threadIdx.x * PKS_ITEMS;
    long long v = 0; size_t idx;
    for (int i = 0; i < PKS_ITEMS; i++) if (j0 + i < n) v += pks_size(q, j0 + i, &idx);
    long long all;
    (void)pks_block_scan(v, sh, &all);
    if (threadIdx.x == 0) bsum[blockIdx.x] = all;
}
/* one workgroup: the tile sums -> the tiles' bases (in place), and the call's total */
extern "C" __global__ void __launch_bounds__(PKS_THREADS) lc3_pack_base_kernel(long long* __restrict__ bsum, long long nb, long long* __restrict__ total)
{
    __shared__ long long sh[PKS_THREADS];
    long long run = 0;
    for (long long b0 = 0; b0 < nb; b0 += PKS_THREADS) {
        const long long b = b0 + threadIdx.x;
        const long long v = b < nb ? bsum[b] : 0;
        long long all;
        const long long ex = pks_block_scan(v, sh, &all);
        if (b < nb) bsum[b] = run + ex;
        run += all;
    }
    if (threadIdx.x == 0 && total) *total = run;
}
/* every frame's offset: into the writers' table (-1 where the frame does not fit cap: lc3d_pack_fits) and the caller's offsets; flag bit
 * LC3D_ENC_FL_PACK_CAP beside the plan kernel's bits (plan_flags) or alone; the sizes into num_bytes when no plan kernel wrote them */
extern "C" __global__ void __launch_bounds__(PKS_THREADS) lc3_pack_offsets_kernel(PkSrc q, long long n, const long long* __restrict__ base, long long cap,
                                                                              long long* __restrict__ tab, long long* __restrict__ offsets,
                                                                              uint8_t* __restrict__ flags, int plan_flags, int32_t* __restrict__ num_bytes)
{
    __shared__ long long sh[PKS_THREADS];
    const long long j0 = (long long)blockIdx.x * PKS_TILE + (long long)threadIdx.x * PKS_ITEMS;
    int sz[PKS_ITEMS]; size_t ix[PKS_ITEMS];
    long long v = 0;
#pragma unroll
    for (int i = 0; i < PKS_ITEMS; i++) { sz[i] = j0 + i < n ? pks_size(q, j0 + i, &ix[i]) : 0; v += sz[i]; }
    long long all;
    long long off = base[blockIdx.x] + pks_block_scan(v, sh, &all);
#pragma unroll
    for (int i = 0; i < PKS_ITEMS; i++) {
        if (j0 + i >= n) break;
        const size_t k = ix[i];
        const int fit = lc3d_pack_fits(off, sz[i], cap);
        tab[k] = fit ? off : -1;
        if (offsets) offsets[k] = off;
        if (flags) flags[k] = (uint8_t)((plan_flags ? flags[k] : 0) | (fit ? 0 : LC3D_ENC_FL_PACK_CAP));
        if (num_bytes) num_bytes[k] = sz[i];
        off += sz[i];
    }
}

/* Tail kernel, behind the call's last kernel: one channel-stream per lane configures its channel from the stream's carry after the call (pend), as the host
 * configures it after encode_bitrates / encode_bandwidths.  With rates (all): the channel's share of the bytes from etab (derive_chan), its payload
 * offset, the bandwidth words and the rate.  Without: the bandwidth words alone.  Either way the pending one-shot attack-detector reset is cleared: the
 * call's kernels have done it. */
extern "C" __global__ void __launch_bounds__(WAVE) lc3_enc_rates_tail_kernel(const int4* __restrict__ pend, const lc3d_chan* __restrict__ etab, lc3d_chan* __restrict__ chans,
                                                                             int channels, int ncs, int dms, int all)
{
    const int cs = (int)(blockIdx.x * WAVE + threadIdx.x);
    if (cs >= ncs) return;
    const int strm = cs / channels, ch = cs - strm * channels;
    const int4 e = pend[strm];
    lc3d_chan* d = chans + cs;
    if (all) {
        const int fb = e.y;
        lc3d_chan v = etab[channels == 1 ? fb : ch ? fb >> 1 : (fb + 1) >> 1];
        v.out_off = ch ? (fb + 1) >> 1 : 0;
        v.bandwidth = e.z; v.bw_cut_bin = lc3d_bw_cut_bin(e.z, dms); v.bw_index = lc3d_bw_index(e.z);
        v.reset_attack = 0; v.bitrate = e.x;
        *d = v;
    } else {
        d->bandwidth = e.z; d->bw_cut_bin = lc3d_bw_cut_bin(e.z, dms); d->bw_index = lc3d_bw_index(e.z);
        d->reset_attack = 0;
    }
}
/* test hook (tests/test_gpu_parity.py::test_device_fastmath_equals_host): lc3_fastmath.h as the kernels evaluate it, over an array.  kind 0 log2, 1 log10, 2 2^x;
 * and the calls that go through the device library's pow: kind 3 m_powf(2, x) (the regulariser, the decoder's SNS gains), kind 4 m_powf(x, k) with k = i mod 9 (the
 * LPC weighting's alpha^k: the array holds every x nine times) */
extern "C" __global__ void lc3_fastmath_test_kernel(int kind, const float* __restrict__ x, float* __restrict__ y, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (kind == 3) y[i] = m_powf(2.0f, x[i]);
    else if (kind == 4) y[i] = m_powf(x[i], (float)(int)(i % 9));
    else y[i] = kind == 0 ? m_log2f(x[i]) : kind == 1 ? m_log10f(x[i]) : m_pow2f(x[i]);
}
