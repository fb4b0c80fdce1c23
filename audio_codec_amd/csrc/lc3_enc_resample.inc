/* lc3_enc_resample.inc -- the 12.8 kHz resampler for every shape, two outputs per lane (described in lc3_enc_pre.inc, which includes this file).
 *
 * RESAMPLE_PCM_FMT 0: lc3_enc_resample_kernel for the reference's three PCM formats (16, 24, 32 in the default layout), token for token what it was before the PCM
 * format word existed.  RESAMPLE_PCM_FMT 1 (the -DLC3_PCM_FMT object): lc3_enc_resample_fmt_kernel for the formats beyond those (float samples, the interleaved and the channel-major layout,
 * lc3_plan.h: lc3d_pcm_*); the two differ in the PCM load alone. */
#if RESAMPLE_PCM_FMT
#define RESAMPLE_FN ERP_FN(LC3_RESAMPLE_FMT_FN)
#else
#define RESAMPLE_FN ERP_FN(lc3_enc_resample_kernel)
#endif
extern "C" __global__ void __launch_bounds__(WAVE)
RESAMPLE_FN(const lc3d_plan* __restrict__ P, const float* __restrict__ state, int state_words, int memcap, const void* __restrict__ pcm, int bitdepth,
                        int T, int tb, int nt, int ncs, float* __restrict__ d12 /* [cs][T][128] */,
                        const float* __restrict__ xprev /* the MDCT / resampler memory before frame 0 (slot of memcap words per channel-stream) */, int xprev_stride LC3_PLACED_OPT LC3_ERP_OPT)
{
    __shared__ PreLds L;
    const int lane = threadIdx.x;
    const int runs = (nt + PRE_FPW - 1) / PRE_FPW;
#ifdef LC3_ENC_RPIPE                /* ragged: the run ends at the stream's count; a wave with nothing left loads nothing */
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * PRE_FPW;
    if (cs >= ncs) return;
    const int t1 = imin(imin(tb + nt, t0 + PRE_FPW), cnt[cs / P->channels]);
    if (t0 >= t1) return;
#else
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * PRE_FPW, t1 = imin(tb + nt, t0 + PRE_FPW);
    if (cs >= ncs) return;
#endif
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    for (int i = lane; i < 240; i += WAVE) L.taps[i] = P->rs_taps[i];
    LSYNC();
    const int mlen = PI(rs_mem_in_len), stride = PI(rs_stride), n12 = PI(n12), N = PI(N), channels = PI(channels);
    const float sf = PF(rs_scale);
    const int strm = cs / channels, ch = cs - strm * channels;
    const int Tt = 240 / stride;
    int n0 = lane, n1 = lane + 64;                  /* the two outputs of this lane (same filter phase: 15 x 64 is a multiple of every stride) */
    if (stride == 4 && n12 == 128) { n0 = lc3t_rs48_map[lane]; n1 = lc3t_rs48_map[64 + lane]; }
    const int i0 = 15 * n0, i1 = 15 * n1, r = i0 % stride, start = r ? stride - r : 0;
    const float* tp = &L.taps[start * Tt];
    const bool on0 = n0 < n12, on1 = n1 < n12;
    float* xs = L.xs;
    /* the PCM of a frame (16 bytes per lane when the layout allows) is requested one frame ahead: the wave has nothing else to hide the round trip with */
#if !RESAMPLE_PCM_FMT
    const bool fast16 = bitdepth == 16 && (N & 7) == 0 && N <= 8 * WAVE && ((((size_t)pcm) + (((size_t)strm * T) * channels + ch) * N * 2) & 15) == 0 && ((N * 2 * channels) & 15) == 0;
    uint4 nv = make_uint4(0, 0, 0, 0);
    if (fast16 && t0 < t1 && lane < (N >> 3)) nv = ((const uint4*)((const int16_t*)pcm + (((size_t)strm * T + t0) * channels + ch) * N))[lane];
#endif
    for (int t = t0; t < t1; t++) {
#if !RESAMPLE_PCM_FMT
        const size_t fidx = ((size_t)strm * T + t) * channels + ch;
#endif
        /* the previous frame's last mlen samples: from the PCM of this launch, or from the stream's MDCT memory for its first frame */
#ifdef LC3_PCM_PLACED
        if (t > 0) pcm_placed_load<false>(pcm, bitdepth, plo, plcap, channels, N, (size_t)strm * T + t - 1, ch, N - mlen, mlen, xs, lane, sf);
        else for (int j = lane; j < mlen; j += WAVE) xs[j] = xprev[(size_t)cs * xprev_stride + (memcap - mlen + j)] * sf;
        pcm_placed_load<false>(pcm, bitdepth, plo, plcap, channels, N, (size_t)strm * T + t, ch, 0, N, xs + mlen, lane, sf);
#elif RESAMPLE_PCM_FMT
        {                                                          /* by the format word (lc3_plan.h): a frame's first element and the step between its samples */
            const int ps = lc3d_pcm_stride(bitdepth, channels);
            const size_t pf = lc3d_pcm_frame(bitdepth, channels, T, N, strm, t, ch), pp = t > 0 ? lc3d_pcm_frame(bitdepth, channels, T, N, strm, t - 1, ch) : 0;
            for (int j = lane; j < mlen; j += WAVE) {
                float v;
                if (t > 0) v = PCM_IN(pcm, bitdepth, pp + (size_t)(N - mlen + j) * ps);
                else v = xprev[(size_t)cs * xprev_stride + (memcap - mlen + j)];
                xs[j] = v * sf;
            }
            if (PCM_F32_WIDE(pcm, bitdepth, pf, N)) {              /* float samples one after the other: 16 bytes per lane */
                const float4* p = (const float4*)((const float*)pcm + pf);
                for (int i = lane; i < (N >> 2); i += WAVE) {
                    const float4 v = pcm_f32x4(p[i]);
                    float* d = &xs[mlen + 4 * i];
                    d[0] = v.x * sf; d[1] = v.y * sf; d[2] = v.z * sf; d[3] = v.w * sf;
                }
            } else for (int j = PCM_RUN(false, pcm, bitdepth, pf, N, xs + mlen, lane, sf) + lane; j < N; j += WAVE) xs[mlen + j] = PCM_IN(pcm, bitdepth, pf + (size_t)j * ps) * sf;
        }
#else
        if (t > t0 && fast16) {
            for (int j = lane; j < mlen; j += WAVE) xs[j] = xs[N + j];          /* still in LDS: the tail of the frame before */
        } else {
            for (int j = lane; j < mlen; j += WAVE) {
                float v;
                if (t > 0) v = pre_pcm(pcm, bitdepth, (fidx - channels) * N + (N - mlen + j));
                else v = xprev[(size_t)cs * xprev_stride + (memcap - mlen + j)];
                xs[j] = v * sf;
            }
        }
        if (fast16) {
            LSYNC();
            if (lane < (N >> 3)) {
                const uint4 v = nv;
                float* d = &xs[mlen + 8 * lane];
                d[0] = (float)(int16_t)(v.x & 0xffff) * sf; d[1] = (float)(int16_t)(v.x >> 16) * sf;
                d[2] = (float)(int16_t)(v.y & 0xffff) * sf; d[3] = (float)(int16_t)(v.y >> 16) * sf;
                d[4] = (float)(int16_t)(v.z & 0xffff) * sf; d[5] = (float)(int16_t)(v.z >> 16) * sf;
                d[6] = (float)(int16_t)(v.w & 0xffff) * sf; d[7] = (float)(int16_t)(v.w >> 16) * sf;
            }
            if (t + 1 < t1 && lane < (N >> 3)) nv = ((const uint4*)((const int16_t*)pcm + (fidx + channels) * N))[lane];
        } else if (bitdepth == 16 && (N & 7) == 0 && ((((size_t)pcm) + fidx * N * 2) & 15) == 0) {      /* 16 bytes per lane */
            const uint4* p = (const uint4*)((const int16_t*)pcm + fidx * N);
            for (int i = lane; i < (N >> 3); i += WAVE) {
                const uint4 v = p[i];
                float* d = &xs[mlen + 8 * i];
                d[0] = (float)(int16_t)(v.x & 0xffff) * sf; d[1] = (float)(int16_t)(v.x >> 16) * sf;
                d[2] = (float)(int16_t)(v.y & 0xffff) * sf; d[3] = (float)(int16_t)(v.y >> 16) * sf;
                d[4] = (float)(int16_t)(v.z & 0xffff) * sf; d[5] = (float)(int16_t)(v.z >> 16) * sf;
                d[6] = (float)(int16_t)(v.w & 0xffff) * sf; d[7] = (float)(int16_t)(v.w >> 16) * sf;
            }
        } else for (int j = lane; j < N; j += WAVE) xs[mlen + j] = pre_pcm(pcm, bitdepth, fidx * N + j) * sf;
#endif
        LSYNC();
        /* polyphase FIR, R/resamp12k8.c:48-57: the taps of a lane's phase 10 at a time, both outputs of the lane share them */
        const float* b0 = on0 ? xs + (i0 + start) / stride : xs;
        const float* b1 = on1 ? xs + (i1 + start) / stride : xs;
        float m0 = 0, m1 = 0;
        for (int tb = 0; tb < Tt; tb += 10) {
            float tap[10];
#pragma unroll
            for (int m = 0; m < 10; m++) tap[m] = tp[tb + m];
#pragma unroll
            for (int m = 0; m < 10; m++) { m0 += b0[tb + m] * tap[m]; m1 += b1[tb + m] * tap[m]; }
        }
        float* o = d12 + ((size_t)cs * T + t) * 128;
        if (on0) o[n0] = m0;
        if (on1) o[n1] = m1;
        LSYNC();
    }
}
#undef RESAMPLE_FN
