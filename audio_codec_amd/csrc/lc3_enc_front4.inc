/* lc3_enc_front4.inc -- the stateless front for N = 480 (48 kHz / 10 ms), FOUR consecutive frames of a stream per wave (included by lc3_kernels.hip).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  Same arithmetic, operation for operation, as lc3_enc_front_kernel's stages
 * (window + fold R/mdct.c:113-119, pre-twiddle R/dct4.c:84-86, 240-point DFT as 15 x 16 R/fft/fft_240_480.h:16-88 with the kernels of
 * R/fft/fft_15_16.h, post-twiddle R/dct4.c:90-94), mapped so that the lanes are busy: one frame's 15 transforms of length 16 and 16 of length 15
 * keep 30 and 16 lanes of a wave busy (lc3_enc_front_kernel: 0.52 of the lanes enabled on average), four frames' keep 60 and 64.
 *
 *   x[]  = [MDCT memory | frame 0 | frame 1 | frame 2 | frame 3] as floats: frame f's window input t_f starts 480 f words in (the memory of
 *          frame f + 1 IS the tail of frame f), so nothing slides.
 *   fold + pre-twiddle: lane l < 60 owns DFT inputs i = l + 60 k (k < 4) of all four frames - window and twiddle values are loaded once for
 *          four frames; the two folded values an input needs are computed from x directly (i < 120: real part from the first fold form, imaginary
 *          from the second; i >= 120 the other way round), into registers; then x is dead and becomes the work buffer:
 *   Z_f[col][l] (col = i mod 15, l = i mod 16; 36 words per column, 544 per frame: conflict-free for both DFT passes)
 *   columns: lane = 16 f + col does one whole 16-point transform in place (8 x 128-bit reads, 8 writes);
 *   rows:    lane = 16 f + row does one 15-point transform and the post-twiddle of its 15 bins, scatters them to natural order in A_f = x + 480 f;
 *   out:     frames t0 .. t0+3 of a chunk of 16 lines are 256 consecutive bytes of the tiled rows (lc3_plan.h LC3D_ROW_BASE): 128-bit stores.
 * The attack detector's block energies (R/attack_detector.c:26-77; 32 / 48 kbps streams only) are taken frame by frame before the fold. */
#define F4_FR 4
#define F4_N 480
#define F4_CS 36            /* words between two columns of Z */
#define F4_ZS 544           /* words between the work buffers of two frames (= 32 mod 64 banks) */
struct __attribute__((aligned(16))) Front4Lds {
    float x[MEMCAP + F4_FR * F4_N + 4];
    float scr[364];         /* attack detector scratch */
    int   pc[LC3D_PLAN_HEAD_WORDS];
    int   cc[14];
};
static_assert(MEMCAP % 4 == 0 && F4_FR * F4_ZS <= MEMCAP + F4_FR * F4_N, "front4 work buffers fit into the PCM area");

/* The 240-point DFT of four frames (15 x 16 prime-factor, R/fft/fft_240_480.h:16-88) and the post-twiddle of the DCT-IV (R/dct4.c:90-94), shared with the
 * decoder's lc3_dec_imdct4_kernel.  in: Z_f[col][l] at x + F4_ZS f (pre-twiddled DFT inputs); out: the 480 values of frame f in natural order at x + 480 f. */
__device__ __forceinline__ void f4_dft240x4(float* x, const lc3d_plan* __restrict__ P, float norm, int lane)
{
    constexpr int N = F4_N;
    /* ---- 15 transforms of length 16 per frame (R/fft/fft_240_480.h:30-52): lane = 16 f + col, in place ---- */
    {
        const int f = lane >> 4, col = lane & 15;
        if (col < 15) {
            float* z = &x[F4_ZS * f + F4_CS * col];
            float v[32];
#pragma unroll
            for (int q = 0; q < 8; q++) { const float4 u = *(const float4*)&z[4 * q]; v[4 * q] = u.x; v[4 * q + 1] = u.y; v[4 * q + 2] = u.z; v[4 * q + 3] = u.w; }
            dft16(v);
#pragma unroll
            for (int q = 0; q < 8; q++) *(float4*)&z[4 * q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        }
    }
    LSYNC();
    /* ---- 16 transforms of length 15 per frame (:54-86) + post-twiddle (R/dct4.c:90-94): lane = 16 f + row ---- */
    {
        const int f = lane >> 4, row = lane & 15;
        float v[30];
#pragma unroll
        for (int l = 0; l < 15; l++) { const float2 u = *(const float2*)&x[F4_ZS * f + F4_CS * l + 2 * row]; v[2 * l] = u.x; v[2 * l + 1] = u.y; }
        dft15(v);
        float o0[15], o1[15];
#pragma unroll
        for (int l = 0; l < 15; l++) {
            const unsigned tt = 15u * row + 16u * l, d = tt < tt - 240u ? tt : tt - 240u;        /* (15 row + 16 l) mod 240 */
            const float2 tw = *(const float2*)&P->tw2[2 * d];
            const float ar = v[2 * l], ai = v[2 * l + 1];
            const float tr = ar * tw.x - ai * tw.y, ti = ai * tw.x + ar * tw.y;
            o0[l] = tr * norm; o1[l] = -ti * norm;
        }
        LSYNC();
        float* A = &x[N * f];
#pragma unroll
        for (int l = 0; l < 15; l++) {
            const unsigned tt = 15u * row + 16u * l, d = tt < tt - 240u ? tt : tt - 240u;
            A[2 * d] = o0[l]; A[N - 2 * d - 1] = o1[l];
        }
    }
    LSYNC();
}

#ifndef LC3_TU_DEC_RAGGED         /* the decoder's ragged object takes the transform above and no encoder kernel */
#ifndef F4_WAVES
#define F4_WAVES 4
#endif
extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(F4_WAVES, F4_WAVES)))
#ifdef LC3_PCM_FMT               /* the object of the PCM formats beyond 16 / 24 / 32 (float samples, the interleaved and the channel-major layout): the PCM load differs, nothing else */
ERP_FN(LC3_FMT_CAT(lc3_enc_front4_kernel))(
#else
ERP_FN(lc3_enc_front4_kernel)(
#endif
                      const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, const float* __restrict__ state, const void* __restrict__ pcm, int bitdepth,
                      int T, int tb, int nt /* frames tb ... tb + nt - 1 of the call's T */, int ncs, float* __restrict__ spec, int srow, int RT, int r0, float* __restrict__ rec,
                      float* __restrict__ xnext, const float* __restrict__ xprev, int xprev_stride LC3_PLACED_OPT LC3_ERP_OPT)
{
    __shared__ Front4Lds L;
    const int lane = threadIdx.x;
    const int runs = (nt + F4_FR - 1) / F4_FR;
#ifdef LC3_ENC_RPIPE                /* ragged: the group ends at the stream's count tend, and the wave that holds frame tend - 1 hands the MDCT memory over */
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * F4_FR;
    if (cs >= ncs) return;
    const int tend = cnt[cs / P->channels], nf = imin(imin(F4_FR, tb + nt - t0), tend - t0);
    if (nf <= 0) return;
#else
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * F4_FR, nf = imin(F4_FR, tb + nt - t0), tend = T;
    if (cs >= ncs) return;
#endif
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    if (lane < 14) L.cc[lane] = ((const int*)&chans[cs])[lane];
    LSYNC();
    constexpr int N = F4_N, h = N / 2;
    const int channels = PI(channels);
    const int strm = cs / channels, ch = cs - strm * channels;
#ifndef LC3_PCM_FMT
    const float sc = bitdepth == 24 ? 256.0f : 65536.0f;
#endif
#ifdef LC3_PCM_PLACED
    /* ---- PCM of the run and the MDCT memory in front of it -> x: every frame at its own offset ---- */
    if (t0 == 0) { for (int i = lane; i < MEMCAP; i += WAVE) L.x[i] = xprev[(size_t)cs * xprev_stride + i]; }
    else pcm_placed_load<true>(pcm, bitdepth, plo, plcap, channels, N, (size_t)strm * T + t0 - 1, ch, N - MEMCAP, MEMCAP, L.x, lane, 1.0f);
    for (int f = 0; f < nf; f++) pcm_placed_load<true>(pcm, bitdepth, plo, plcap, channels, N, (size_t)strm * T + t0 + f, ch, 0, N, &L.x[MEMCAP + N * f], lane, 1.0f);
#elif defined(LC3_PCM_FMT)
    /* ---- PCM of the run and the MDCT memory in front of it -> x ---- */
    {   /* by the format word: the run's first element, the step to the next sample and to the channel's next frame.  Float samples that follow each other (480 x 4
         * bytes per frame from a 16-byte aligned base) take 16 bytes per lane like the 16-bit ones of the kernel without the suffix. */
        const int ps = lc3d_pcm_stride(bitdepth, channels);
        const size_t pf0 = lc3d_pcm_frame(bitdepth, channels, T, N, strm, t0, ch), pfst = lc3d_pcm_fstep(bitdepth, channels, N);
        const bool fastf = PCM_F32_WIDE(pcm, bitdepth, pf0, N) && ((pfst * 4) & 15) == 0;
        if (t0 == 0) { for (int i = lane; i < MEMCAP; i += WAVE) L.x[i] = xprev[(size_t)cs * xprev_stride + i]; }
        else {
            const size_t pidx = pf0 - pfst + (size_t)(N - MEMCAP) * ps;
            if (fastf) {
                const float4* p = (const float4*)((const float*)pcm + pidx);
                for (int j = lane; j < MEMCAP / 4; j += WAVE) *(float4*)&L.x[4 * j] = pcm_f32x4(p[j]);
            } else for (int j = PCM_RUN(true, pcm, bitdepth, pidx, MEMCAP, L.x, lane, 1.0f) + lane; j < MEMCAP; j += WAVE) L.x[j] = PCM_IN(pcm, bitdepth, pidx + (size_t)j * ps);
        }
        if (fastf) {
            for (int idx = lane; idx < 120 * nf; idx += WAVE) {                          /* 120 x 16 bytes per frame */
                const int f = idx / 120, j = idx - 120 * f;
                *(float4*)&L.x[MEMCAP + N * f + 4 * j] = pcm_f32x4(((const float4*)((const float*)pcm + pf0 + (size_t)f * pfst))[j]);
            }
        } else {
            for (int f = 0; f < nf; f++) {
                const size_t o = pf0 + (size_t)f * pfst;
                for (int i = PCM_RUN(true, pcm, bitdepth, o, N, &L.x[MEMCAP + N * f], lane, 1.0f) + lane; i < N; i += WAVE) L.x[MEMCAP + N * f + i] = PCM_IN(pcm, bitdepth, o + (size_t)i * ps);
            }
        }
    }
#else
    /* ---- PCM of the run and the MDCT memory in front of it -> x ---- */
    {
        const size_t f0 = ((size_t)strm * T + t0) * channels + ch;
        const bool fast = bitdepth == 16 && (((size_t)pcm) & 15) == 0;
        if (t0 == 0) { for (int i = lane; i < MEMCAP; i += WAVE) L.x[i] = xprev[(size_t)cs * xprev_stride + i]; }
        else {
            const size_t pidx = (f0 - channels) * N + (N - MEMCAP);
            if (fast) {
                const uint2* p = (const uint2*)((const int16_t*)pcm + pidx);
                for (int j = lane; j < MEMCAP / 4; j += WAVE) {
                    const uint2 v = p[j];
                    *(float4*)&L.x[4 * j] = make_float4((float)(int16_t)(v.x & 0xffff), (float)(int16_t)(v.x >> 16), (float)(int16_t)(v.y & 0xffff), (float)(int16_t)(v.y >> 16));
                }
            } else for (int j = lane; j < MEMCAP; j += WAVE)
                L.x[j] = bitdepth == 16 ? (float)((const int16_t*)pcm)[pidx + j] : (float)((const int32_t*)pcm)[pidx + j] / sc;
        }
        if (fast) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int idx = lane + 64 * k, f = idx / 60, j = idx - 60 * f;           /* 60 x 16 bytes per frame */
                if (idx < 240 && f < nf) {
#ifdef F4_NOLOAD      /* diagnostic (tools/variants.sh): what the kernel costs without its PCM round trip - the output of such a build is not the encoder's */
                    const uint4 v = make_uint4(idx * 77u, idx * 131u, idx * 17u, idx * 3u);
#else
                    const uint4 v = ((const uint4*)((const int16_t*)pcm + (f0 + (size_t)f * channels) * N))[j];
#endif
                    float* d = &L.x[MEMCAP + N * f + 8 * j];
                    *(float4*)&d[0] = make_float4((float)(int16_t)(v.x & 0xffff), (float)(int16_t)(v.x >> 16), (float)(int16_t)(v.y & 0xffff), (float)(int16_t)(v.y >> 16));
                    *(float4*)&d[4] = make_float4((float)(int16_t)(v.z & 0xffff), (float)(int16_t)(v.z >> 16), (float)(int16_t)(v.w & 0xffff), (float)(int16_t)(v.w >> 16));
                }
            }
        } else {
            for (int f = 0; f < nf; f++) {
                const size_t o = (f0 + (size_t)f * channels) * N;
                for (int i = lane; i < N; i += WAVE)
                    L.x[MEMCAP + N * f + i] = bitdepth == 16 ? (float)((const int16_t*)pcm)[o + i] : (float)((const int32_t*)pcm)[o + i] / sc;
            }
        }
    }
#endif
    LSYNC();
    if (t0 + nf == tend) for (int i = lane; i < MEMCAP; i += WAVE) xnext[(size_t)cs * MEMCAP + i] = L.x[N * nf + i];     /* the MDCT memory behind the call's last frame */
    float* r = rec + ((size_t)cs * RT + r0 + t0) * FR_WORDS;
    if (lane < nf) ((int*)r)[(size_t)lane * FR_WORDS + FR_ATTFLAG] = 0;   /* lc3_enc_attack_kernel sets the flag where the detector runs */
    /* ---- attack detector, first half: frame by frame (its filter memory entering a frame = the last two 16 kHz samples before it) ---- */
    if (CI(attack_handling) != 0) {
        const float* stp = state + (size_t)cs * LC3D_STATE_WORDS(MEMCAP);
        float am0 = 0, am1 = 0;
        for (int f = 0; f < nf; f++) {
            if (t0 + f == 0) { if (!CI(reset_attack)) { am0 = stp[LC3D_ST_SCAL(MEMCAP) + F_ATT_M0]; am1 = stp[LC3D_ST_SCAL(MEMCAP) + F_ATT_M1]; } }
            else if (f == 0) { const float* q = &L.x[MEMCAP]; am0 = (q[-6] + q[-5] + q[-4]); am1 = (q[-3] + q[-2] + q[-1]); }      /* 48 kHz */
            float n0, n1;
            const float e = attack_energies_at(PI(att_nblocks), 48000, &L.x[MEMCAP + N * f], L.scr, lane, am0, am1, n0, n1);
            float* rf = r + (size_t)f * FR_WORDS;
            if (lane < 4) rf[FR_ATT + lane] = lane < PI(att_nblocks) ? e : 0.0f;
            if (lane == 0) { rf[FR_ATTM] = n0; rf[FR_ATTM + 1] = n1; }
            am0 = n0; am1 = n1;
            LSYNC();
        }
    }
    /* ---- window + fold + pre-twiddle: x -> registers ---- */
    const float* w = &lc3t_win_pool[PI(win_off)];
    const int lim = 2 * N - PI(la);
    float zr[4][F4_FR], zi[4][F4_FR];
    if (lane < 60) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = lane + 60 * k;
            /* fold form 1 (R/mdct.c:116): F[m] = -t[3h-m-1] w[3h-m-1] - t[3h+m] w[3h+m];  form 2 (:117): F[h+m] = t[m] w[m] - t[2h-m-1] w[2h-m-1];  DFT input i = (F[2i], F[N-2i-1]) x tw1[i] */
            const int m1 = k < 2 ? 2 * i : N - 1 - 2 * i, m2 = k < 2 ? h - 1 - 2 * i : 2 * i - h;
            const int j0 = 3 * h - m1 - 1, j1 = 3 * h + m1, j2 = m2, j3 = 2 * h - m2 - 1;
            const float w0 = w[j0], w1 = w[j1], w2 = w[j2], w3 = w[j3];
            const float2 tw = *(const float2*)&P->tw1[2 * i];
            const bool in1 = j1 < lim; const int j1c = in1 ? j1 : 0;
#pragma unroll
            for (int f = 0; f < F4_FR; f++) {
                const float* t = &L.x[N * f];
                const float a0 = t[j0] * w0;
                const float a1 = (in1 ? t[j1c] : 0.0f) * w1;
                const float a2 = t[j2] * w2;
                const float a3 = t[j3] * w3;
                const float F1 = -a0 - a1, F2 = a2 - a3;
                const float ar = k < 2 ? F1 : F2, ai = k < 2 ? F2 : F1;
                zr[k][f] = ar * tw.x - ai * tw.y;
                zi[k][f] = ai * tw.x + ar * tw.y;
            }
        }
    }
    LSYNC();
    if (lane < 60) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = lane + 60 * k;
            const int o = (i % 15) * F4_CS + 2 * (i & 15);
#pragma unroll
            for (int f = 0; f < F4_FR; f++) *(float2*)&L.x[F4_ZS * f + o] = make_float2(zr[k][f], zi[k][f]);
        }
    }
    LSYNC();
    f4_dft240x4(L.x, P, PF(dct4_norm), lane);
    /* ---- the coded lines -> tiled rows ---- */
    {
        const int nq = PI(ylen);                             /* ylen / 16 chunks x 4 frames x 4 quads */
        float* base = LC3D_ROW_BASE(spec, cs, r0 + t0, RT, srow);
        for (int idx = lane; idx < nq; idx += WAVE) {
            const int c = idx >> 4, f = (idx >> 2) & 3, q = idx & 3;
            if (f < nf) *(float4*)&base[((size_t)c * RT + f) * 16 + 4 * q] = *(const float4*)&L.x[N * f + 16 * c + 4 * q];
        }
    }
}
#endif /* !LC3_TU_DEC_RAGGED */
