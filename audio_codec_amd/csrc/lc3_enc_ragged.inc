/* lc3_enc_ragged.inc -- the small kernels of the encoder's ragged calls (include/lc3plus_batch.h: lc3plus_enc_batch_set_frame_counts), alone in the _eplan object of
 * lc3_kernels.hip (which includes this file) so that the object of their dense twins (lc3_util_kernels.inc) stays what it is.  The one-wave kernel's ragged form is
 * lc3_enc_wave.inc with -DLC3_ENC_RAGGED. */

/* lc3_enc_plan_rates_kernel with per-stream frame counts: one stream per lane.  It clamps counts[s] into cnt[s] - the one place the caller's counts are read; every
 * other kernel of the call reads cnt - walks the rule of lc3d_enc_frame_step over the stream's first c = cnt[s] frames, and writes for every frame of the call what
 * the ragged one-wave kernel and the packed scan take: fsz ALWAYS (the carried bytes where the caller gave no rates: the kernel has per-frame sizes whatever the
 * call), bwf with bandwidths, and with tab (slotted output) the frame's place (s T + t) out_stride in the table a packed call's scan fills instead.  An absent
 * frame (t >= c) gets size 0, num_bytes 0 and flags LC3D_ENC_FL_ABSENT; its rate and bandwidth take no part in anything (the four-frame path loads the group a
 * present frame lies in, whole - the arrays hold T entries per stream - and steps the present ones).  carry and pend hold the values after frame c - 1: those
 * before the call where c is 0. */
extern "C" __global__ void __launch_bounds__(WAVE) lc3_enc_plan_rates_kernel_rag(lc3d_rate_rule r, const int32_t* __restrict__ rates, const int32_t* __restrict__ bws,
                                                                                 int T, int n_streams, int4* __restrict__ carry, const lc3d_chan* __restrict__ seed,
                                                                                 uint16_t* __restrict__ fsz, uint16_t* __restrict__ bwf, int32_t* __restrict__ num_bytes,
                                                                                 uint8_t* __restrict__ flags, int4* __restrict__ pend, int vec4,
                                                                                 const int32_t* __restrict__ counts, int32_t* __restrict__ cnt,
                                                                                 long long* __restrict__ tab, int out_stride)
{
    const int s = (int)(blockIdx.x * WAVE + threadIdx.x);
    if (s >= n_streams) return;
    const int c = lc3d_dec_count_clamp(counts[s], T);
    cnt[s] = c;
    int rate, bytes, bw;
    if (seed) {
        const lc3d_chan* ch = seed + (size_t)s * r.channels;
        rate = ch[0].bitrate; bw = ch[0].bandwidth; bytes = ch[0].nbytes;
        if (r.channels > 1) bytes += ch[1].nbytes;
    } else { const int4 e = carry[s]; rate = e.x; bytes = e.y; bw = e.z; }
    const size_t row = (size_t)s * T;
    /* one frame: the rule where it is present, the absent values where it is not (br, bv: whatever was loaded, unused then) */
    auto step = [&](int t, int br, int bv, int* z, int* w) {
        if (t >= c) { *z = 0; *w = 0; return (int)LC3D_ENC_FL_ABSENT; }
        const int f = lc3d_enc_frame_step(&r, rates != nullptr, br, bws != nullptr, bv, &rate, &bytes, &bw);
        *z = bytes; *w = bw;
        return f;
    };
    if (vec4) {
        for (int t = 0; t < T; t += 4) {
            const size_t i = row + t;
            const bool any = t < c;                                /* a group behind the count loads nothing */
            const int4 rv = rates && any ? *(const int4*)(rates + i) : make_int4(0, 0, 0, 0);
            const int4 bv = bws && any ? *(const int4*)(bws + i) : make_int4(0, 0, 0, 0);
            int z0, z1, z2, z3, w0, w1, w2, w3;
            const int f0 = step(t, rv.x, bv.x, &z0, &w0), f1 = step(t + 1, rv.y, bv.y, &z1, &w1), f2 = step(t + 2, rv.z, bv.z, &z2, &w2), f3 = step(t + 3, rv.w, bv.w, &z3, &w3);
            *(uint2*)(fsz + i) = make_uint2((unsigned)z0 | (unsigned)z1 << 16, (unsigned)z2 | (unsigned)z3 << 16);
            if (bws) *(uint2*)(bwf + i) = make_uint2((unsigned)w0 | (unsigned)w1 << 16, (unsigned)w2 | (unsigned)w3 << 16);
            if (num_bytes) *(int4*)(num_bytes + i) = make_int4(z0, z1, z2, z3);
            if (flags) *(unsigned*)(flags + i) = (unsigned)f0 | (unsigned)f1 << 8 | (unsigned)f2 << 16 | (unsigned)f3 << 24;
        }
    } else {
        for (int t = 0; t < T; t++) {
            const size_t i = row + t;
            const bool here = t < c;
            int z, w;
            const int f = step(t, rates && here ? rates[i] : 0, bws && here ? bws[i] : 0, &z, &w);
            fsz[i] = (uint16_t)z;
            if (bws) bwf[i] = (uint16_t)w;
            if (num_bytes) num_bytes[i] = z;
            if (flags) flags[i] = (uint8_t)f;
        }
    }
    if (tab) for (int t = 0; t < T; t++) tab[row + t] = (long long)(row + t) * out_stride;
    const int4 e = make_int4(rate, bytes, bw, 0);
    carry[s] = e; pend[s] = e;
}
/* lc3_enc_rates_tail_kernel behind a ragged call: a stream of which no frame was present keeps its configuration word for word - the one-shot attack-detector
 * reset pending from set_bitrate included, which no kernel has done for it; it takes effect at the stream's first present frame. */
extern "C" __global__ void __launch_bounds__(WAVE) lc3_enc_rates_tail_kernel_rag(const int4* __restrict__ pend, const lc3d_chan* __restrict__ etab,
                                                                                 lc3d_chan* __restrict__ chans, int channels, int ncs, int dms, int all,
                                                                                 const int32_t* __restrict__ cnt)
{
    const int cs = (int)(blockIdx.x * WAVE + threadIdx.x);
    if (cs >= ncs) return;
    const int strm = cs / channels, ch = cs - strm * channels;
    if (cnt[strm] == 0) return;
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
/* Last kernel of a ragged call that reports flags: one stream-frame per lane, an absent frame's flags are exactly LC3D_ENC_FL_ABSENT - whatever the kernels that
 * know nothing of counts (the packed scan's capacity bit, the placement mark) have put beside the plan kernel's value. */
extern "C" __global__ void __launch_bounds__(256) lc3_enc_absent_kernel(const int32_t* __restrict__ cnt, int T, long long n, uint8_t* __restrict__ flags)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long s = i / T;
    if ((int)(i - s * T) >= cnt[s]) flags[i] = (uint8_t)LC3D_ENC_FL_ABSENT;
}
