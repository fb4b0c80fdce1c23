/* lc3_enc_frontm.inc -- the stateless front for the frame lengths whose DFT is a chain of two or three small prime-factor stages
 * (N / 2 in {10, 20, 30, 40, 120}: radices 2, 3, 4, 5, 8), SEVERAL consecutive frames of a stream per wave (included by lc3_kernels.hip).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  The arithmetic is lc3_enc_front_kernel's (mdct_pre / mdct_dft_pfa / mdct_post of
 * lc3_kernels.hip: R/mdct.c:103-124, R/dct4.c:75-95, R/fft/fft_generic.h:634-699 with the leaves of R/fft/fft_2_9.h), operation for operation;
 * what changes is how many lanes work.  A stage of a 120-point DFT is 15 transforms of length 8, 40 of length 3 or 24 of length 5: one frame
 * keeps 15 ... 40 lanes busy, and a 20-point DFT 4 or 5.  Here a wave owns `F` consecutive frames (4 for N = 240, 8 below) and a stage's tasks
 * are (frame, transform) pairs, 64 to a round.  The frames' PCM lies in one LDS array behind the MDCT memory (the memory of frame f + 1 is the
 * tail of frame f: nothing slides); the stages ping-pong between that array and a second one. */
#ifndef FM_CAP
#define FM_CAP 960              /* F x N <= 960 words */
#endif
struct __attribute__((aligned(16))) FrontMLds {
    float x[MEMCAP + FM_CAP];
    float b[FM_CAP];
    float scr[364];             /* attack detector scratch */
    int   pc[LC3D_PLAN_HEAD_WORDS];
    int   cc[14];
};

/* one stage: task tk = (frame f, transform l < cnt): gather RAD complex values of frame f through `map`, transform, write to consecutive slots (or
 * through `dst`).  in / out are different arrays. */
template <int RAD> __device__ __forceinline__ void fm_stage_r(const uint8_t* __restrict__ map, const uint8_t* __restrict__ dst, const float* in, float* out, int cnt, int nf, int N, int lane)
{
    const int ntask = nf * cnt;
    const float rc = 1.0f / (float)cnt;
    for (int t0 = 0; t0 < ntask; t0 += WAVE) {
        const int tk = t0 + lane;
        const bool on = tk < ntask;
        const int f = on ? (int)(((float)tk + 0.5f) * rc) : 0, l = on ? tk - f * cnt : 0;
        const int base = l * RAD;
        const float* inf = in + f * N; float* outf = out + f * N;
        float v[2 * RAD];
#pragma unroll
        for (int j = 0; j < RAD; j++) { const int s = map[base + j]; v[2 * j] = inf[2 * s]; v[2 * j + 1] = inf[2 * s + 1]; }
        if (RAD == 2) { const float r1 = v[0], i1 = v[1], r2 = v[2], i2 = v[3]; v[0] = r1 + r2; v[1] = i1 + i2; v[2] = r1 - r2; v[3] = i1 - i2; }   /* R/fft/fft_2_9.h:22-37 */
        else if (RAD == 3) dft3(v);
        else if (RAD == 4) dft4(v);
        else if (RAD == 5) dft5(v);
        else dft8(v);
        if (on) {
#pragma unroll
            for (int j = 0; j < RAD; j++) { const int d = dst ? dst[base + j] : base + j; outf[2 * d] = v[2 * j]; outf[2 * d + 1] = v[2 * j + 1]; }
        }
    }
    LSYNC();
}
__device__ __forceinline__ void fm_stage(const uint8_t* __restrict__ map, const uint8_t* __restrict__ dst, const float* in, float* out, int rad, int cnt, int nf, int N, int lane)
{
    switch (rad) {                                  /* wave-uniform */
    case 2: fm_stage_r<2>(map, dst, in, out, cnt, nf, N, lane); break;
    case 3: fm_stage_r<3>(map, dst, in, out, cnt, nf, N, lane); break;
    case 4: fm_stage_r<4>(map, dst, in, out, cnt, nf, N, lane); break;
    case 5: fm_stage_r<5>(map, dst, in, out, cnt, nf, N, lane); break;
    default: fm_stage_r<8>(map, dst, in, out, cnt, nf, N, lane); break;
    }
}

extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4, 4)))
#ifdef LC3_PCM_FMT               /* the object of the PCM formats beyond 16 / 24 / 32 (float samples, the interleaved and the channel-major layout): the PCM load differs, nothing else */
ERP_FN(LC3_FMT_CAT(lc3_enc_frontm_kernel))(
#else
ERP_FN(lc3_enc_frontm_kernel)(
#endif
                      const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, const float* __restrict__ state, const void* __restrict__ pcm, int bitdepth,
                      int T, int tb, int nt /* frames tb ... tb + nt - 1 of the call's T */, int F /* frames per wave: F x N <= FM_CAP, F <= 8 */, int ncs,
                      float* __restrict__ spec, int srow, int RT, int r0, float* __restrict__ rec, float* __restrict__ xnext, const float* __restrict__ xprev, int xprev_stride LC3_PLACED_OPT LC3_ERP_OPT)
{
    __shared__ FrontMLds L;
    const int lane = threadIdx.x;
    const int runs = (nt + F - 1) / F;
#ifdef LC3_ENC_RPIPE                /* ragged: the group ends at the stream's count tend, and the wave that holds frame tend - 1 hands the MDCT memory over */
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * F;
    if (cs >= ncs) return;
    const int tend = cnt[cs / P->channels], nf = imin(imin(F, tb + nt - t0), tend - t0);
    if (nf <= 0) return;
#else
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * F, nf = imin(F, tb + nt - t0), tend = T;
    if (cs >= ncs) return;
#endif
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    if (lane < 14) L.cc[lane] = ((const int*)&chans[cs])[lane];
    LSYNC();
    const int N = PI(N), h = N >> 1, la = PI(la), ml = N - la, channels = PI(channels), fs = PI(fs);
    const int strm = cs / channels, ch = cs - strm * channels;
#ifndef LC3_PCM_FMT
    const float sc = bitdepth == 24 ? 256.0f : 65536.0f;
    const size_t f0 = ((size_t)strm * T + t0) * channels + ch;
#endif
#ifdef LC3_PCM_PLACED
    /* ---- the MDCT memory in front of the run (right-aligned below x[MEMCAP]) and the run's PCM -> x: every frame at its own offset ---- */
    if (t0 == 0) { for (int i = lane; i < MEMCAP; i += WAVE) L.x[i] = xprev[(size_t)cs * xprev_stride + i]; }
    else pcm_placed_load<false>(pcm, bitdepth, plo, plcap, channels, N, (size_t)strm * T + t0 - 1, ch, N - ml, ml, &L.x[MEMCAP - ml], lane, 1.0f);
    for (int f = 0; f < nf; f++) pcm_placed_load<true>(pcm, bitdepth, plo, plcap, channels, N, (size_t)strm * T + t0 + f, ch, 0, N, &L.x[MEMCAP + N * f], lane, 1.0f);
#elif defined(LC3_PCM_FMT)
    /* ---- the MDCT memory in front of the run (right-aligned below x[MEMCAP]) and the run's PCM -> x: by the format word - the run's first element, the step to the
     * next sample and to the channel's next frame; float samples that follow each other take 16 bytes per lane like the 16-bit ones of the kernel without the suffix ---- */
    const int ps = lc3d_pcm_stride(bitdepth, channels);
    const size_t pf0 = lc3d_pcm_frame(bitdepth, channels, T, N, strm, t0, ch), pfst = lc3d_pcm_fstep(bitdepth, channels, N);
    if (t0 == 0) { for (int i = lane; i < MEMCAP; i += WAVE) L.x[i] = xprev[(size_t)cs * xprev_stride + i]; }
    else {
        const size_t pidx = pf0 - pfst + (size_t)(N - ml) * ps;
        for (int j = lane; j < ml; j += WAVE) L.x[MEMCAP - ml + j] = PCM_IN(pcm, bitdepth, pidx + (size_t)j * ps);
    }
    if (PCM_F32_WIDE(pcm, bitdepth, pf0, N) && ((pfst * 4) & 15) == 0) {
        const int per = N >> 2, ntask = nf * per;                 /* 16 bytes per lane */
        const float rp = 1.0f / (float)per;
        for (int tk = lane; tk < ntask; tk += WAVE) {
            const int f = (int)(((float)tk + 0.5f) * rp), j = tk - f * per;
            *(float4*)&L.x[MEMCAP + N * f + 4 * j] = pcm_f32x4(((const float4*)((const float*)pcm + pf0 + (size_t)f * pfst))[j]);
        }
    } else {
        for (int f = 0; f < nf; f++) {
            const size_t o = pf0 + (size_t)f * pfst;
            for (int i = PCM_RUN(true, pcm, bitdepth, o, N, &L.x[MEMCAP + N * f], lane, 1.0f) + lane; i < N; i += WAVE) L.x[MEMCAP + N * f + i] = PCM_IN(pcm, bitdepth, o + (size_t)i * ps);
        }
    }
#else
    /* ---- the MDCT memory in front of the run (right-aligned below x[MEMCAP]) and the run's PCM -> x ---- */
    if (t0 == 0) { for (int i = lane; i < MEMCAP; i += WAVE) L.x[i] = xprev[(size_t)cs * xprev_stride + i]; }
    else {
        const size_t pidx = (f0 - channels) * N + (N - ml);
        for (int j = lane; j < ml; j += WAVE)
            L.x[MEMCAP - ml + j] = bitdepth == 16 ? (float)((const int16_t*)pcm)[pidx + j] : (float)((const int32_t*)pcm)[pidx + j] / sc;
    }
    if (bitdepth == 16 && (N & 7) == 0 && (((size_t)pcm) & 15) == 0 && ((N * 2 * channels) & 15) == 0 && (((f0 * N) * 2) & 15) == 0) {
        const int per = N >> 3, ntask = nf * per;                 /* 16 bytes per lane */
        const float rp = 1.0f / (float)per;
        for (int tk = lane; tk < ntask; tk += WAVE) {
            const int f = (int)(((float)tk + 0.5f) * rp), j = tk - f * per;
            const uint4 v = ((const uint4*)((const int16_t*)pcm + (f0 + (size_t)f * channels) * N))[j];
            float* d = &L.x[MEMCAP + N * f + 8 * j];
            d[0] = (float)(int16_t)(v.x & 0xffff); d[1] = (float)(int16_t)(v.x >> 16); d[2] = (float)(int16_t)(v.y & 0xffff); d[3] = (float)(int16_t)(v.y >> 16);
            d[4] = (float)(int16_t)(v.z & 0xffff); d[5] = (float)(int16_t)(v.z >> 16); d[6] = (float)(int16_t)(v.w & 0xffff); d[7] = (float)(int16_t)(v.w >> 16);
        }
    } else {
        for (int f = 0; f < nf; f++) {
            const size_t o = (f0 + (size_t)f * channels) * N;
            for (int i = lane; i < N; i += WAVE)
                L.x[MEMCAP + N * f + i] = bitdepth == 16 ? (float)((const int16_t*)pcm)[o + i] : (float)((const int32_t*)pcm)[o + i] / sc;
        }
    }
#endif
    LSYNC();
    if (t0 + nf == tend) for (int i = lane; i < MEMCAP; i += WAVE) xnext[(size_t)cs * MEMCAP + i] = L.x[N * nf + i];     /* the MDCT memory behind the call's last frame */
    float* r = rec + ((size_t)cs * RT + r0 + t0) * FR_WORDS;
    if (lane < nf) ((int*)r)[(size_t)lane * FR_WORDS + FR_ATTFLAG] = 0;   /* lc3_enc_attack_kernel sets the flag where the detector runs */
    /* ---- attack detector, first half (R/attack_detector.c:26-77), frame by frame ---- */
    if (CI(attack_handling) != 0) {
        const float* stp = state + (size_t)cs * LC3D_STATE_WORDS(MEMCAP);
        float am0 = 0, am1 = 0;
        for (int f = 0; f < nf; f++) {
            if (t0 + f == 0) { if (!CI(reset_attack)) { am0 = stp[LC3D_ST_SCAL(MEMCAP) + F_ATT_M0]; am1 = stp[LC3D_ST_SCAL(MEMCAP) + F_ATT_M1]; } }
            else if (f == 0) {
                const float* q = &L.x[MEMCAP];        /* one past the previous frame's last sample */
                if (fs == 96000) { am0 = q[-12] + q[-11] + q[-10] + q[-9] + q[-8] + q[-7]; am1 = q[-6] + q[-5] + q[-4] + q[-3] + q[-2] + q[-1]; }
                else if (fs == 48000) { am0 = (q[-6] + q[-5] + q[-4]); am1 = (q[-3] + q[-2] + q[-1]); }
                else if (fs == 32000) { am0 = (q[-4] + q[-3]); am1 = (q[-2] + q[-1]); }
                else { am0 = (float)((double)q[-6] + ((double)(q[-5] + q[-4])) / 2.0); am1 = (float)((double)q[-3] + ((double)(q[-2] + q[-1])) / 2.0); }
            }
            float n0, n1;
            const float e = attack_energies_at(PI(att_nblocks), fs, &L.x[MEMCAP + N * f], L.scr, lane, am0, am1, n0, n1);
            float* rf = r + (size_t)f * FR_WORDS;
            if (lane < 4) rf[FR_ATT + lane] = lane < PI(att_nblocks) ? e : 0.0f;
            if (lane == 0) { rf[FR_ATTM] = n0; rf[FR_ATTM + 1] = n1; }
            am0 = n0; am1 = n1;
            LSYNC();
        }
    }
    /* ---- window + fold (R/mdct.c:113-119): x -> b ---- */
    {
        const float* w = &lc3t_win_pool[PI(win_off)];
        const int lim = 2 * N - la, ntask = nf * h;
        const float rh = 1.0f / (float)h;
        for (int tk = lane; tk < ntask; tk += WAVE) {
            const int f = (int)(((float)tk + 0.5f) * rh), i = tk - f * h;
            const float* t = &L.x[MEMCAP - ml + N * f];           /* t[j] = [memory | frame], j < 2N - la; zero beyond */
            const int j0 = 3 * h - i - 1, j1 = 3 * h + i, j2 = i, j3 = 2 * h - i - 1;
            const float a0 = (j0 < lim ? t[j0 < lim ? j0 : 0] : 0.0f) * w[j0];
            const float a1 = (j1 < lim ? t[j1 < lim ? j1 : 0] : 0.0f) * w[j1];
            const float a2 = t[j2] * w[j2];
            const float a3 = t[j3] * w[j3];
            L.b[N * f + i] = -a0 - a1;
            L.b[N * f + h + i] = a2 - a3;
        }
        LSYNC();
        /* pre-twiddle R/dct4.c:84-86: b -> x (frame f at x + N f) */
        for (int tk = lane; tk < ntask; tk += WAVE) {
            const int f = (int)(((float)tk + 0.5f) * rh), i = tk - f * h;
            const float ar = L.b[N * f + 2 * i], ai = L.b[N * f + N - 2 * i - 1], br = P->tw1[2 * i], bi = P->tw1[2 * i + 1];
            L.x[N * f + 2 * i] = ar * br - ai * bi;
            L.x[N * f + 2 * i + 1] = ai * br + ar * bi;
        }
        LSYNC();
    }
    /* ---- the prime-factor stages (R/fft/fft_generic.h:634-699): x -> b (-> x) -> ... ; the last one scatters to natural order ---- */
    float* cur = L.x; float* oth = L.b;
    {
        const int nst = PI(pfa_nst);
        for (int s = 0; s < nst; s++) {
            const int rad = s == 0 ? PI(pfa_rad[0]) : s == 1 ? PI(pfa_rad[1]) : PI(pfa_rad[2]);
            fm_stage(P->pfa_src + s * LC3D_PFA_STRIDE, s == nst - 1 ? P->pfa_dst : nullptr, cur, oth, rad, h / rad, nf, N, lane);
            float* tmp = cur; cur = oth; oth = tmp;
        }
    }
    /* ---- post-twiddle R/dct4.c:90-94: cur -> oth, the spectrum in natural order ---- */
    {
        const float norm = PF(dct4_norm);
        const int ntask = nf * h;
        const float rh = 1.0f / (float)h;
        for (int tk = lane; tk < ntask; tk += WAVE) {
            const int f = (int)(((float)tk + 0.5f) * rh), i = tk - f * h;
            const float ar = cur[N * f + 2 * i], ai = cur[N * f + 2 * i + 1], br = P->tw2[2 * i], bi = P->tw2[2 * i + 1];
            const float tr = ar * br - ai * bi, ti = ai * br + ar * bi;
            oth[N * f + 2 * i] = tr * norm; oth[N * f + N - 2 * i - 1] = -ti * norm;
        }
        LSYNC();
    }
    /* ---- the coded lines -> tiled rows: the same chunk of consecutive frames is adjacent (lc3_plan.h LC3D_ROW_BASE) ---- */
    {
        const int ylen = PI(ylen), nch = (ylen + 15) >> 4;
        float* base = LC3D_ROW_BASE(spec, cs, r0 + t0, RT, srow);
        const int j = lane & 15;
        for (int c = 0; c < nch; c++) {
            for (int fb = 0; fb < nf; fb += 4) {
                const int f = fb + (lane >> 4), k = 16 * c + j;
                if (f < nf && k < ylen) base[((size_t)c * RT + f) * 16 + j] = oth[N * f + k];
            }
        }
    }
}
