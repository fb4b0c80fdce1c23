/* lc3_dec_imdct4.inc -- the decoder's IMDCT for N = 480 (48 kHz / 10 ms), FOUR consecutive frames of a stream per wave (included by lc3_kernels.hip).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  Same arithmetic as lc3_dec_imdct_kernel (SNS shaping R/mdct_shaping.c with the band
 * gains of the parse kernel, or the concealment of a lost frame R/plc_noise_substitution0.c; IMDCT R/imdct.c:13-59 = pre-twiddle, 240-point DFT,
 * post-twiddle R/dct4.c:84-94), mapped like lc3_enc_front4_kernel: one frame's 15 transforms of length 16 and 16 of length 15 keep 30 and 16 lanes
 * of a wave busy, four frames' keep 60 and 64.  The DFT passes and the post-twiddle are f4_dft240x4 of lc3_enc_front4.inc (the DCT-IV is its own
 * inverse: the encoder's and the decoder's transforms are the same code).  The window and the overlap-add belong to the synthesis kernel, as before;
 * this kernel is stateless, all runs of a launch are independent.  Traced launches keep the one-frame-at-a-time kernel. */
struct __attribute__((aligned(16))) Imd4Lds {
    float x[F4_FR * F4_ZS + 16];         /* spectrum A_f at 480 f -> Z_f at 544 f -> time-domain aliasing buffer at 480 f */
    float gi[F4_FR][64];                 /* SNS band gains of the frames */
    int   isc[F4_FR][64];                /* the first 64 record words of the frames */
    unsigned char bsel[F4_N];            /* SNS band of a bin, 255 where the bin is not shaped */
    int   pc[LC3D_PLAN_HEAD_WORDS];
};

#ifndef DEC_IMDCT4_EU
#define DEC_IMDCT4_EU 4
#endif
extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(DEC_IMDCT4_EU, DEC_IMDCT4_EU)))
DEC_RAG(lc3_dec_imdct4_kernel)(const lc3d_plan* __restrict__ P, const float* __restrict__ state, const int* __restrict__ rec /* [cs][T][PR_WORDS] */,
                      const float* __restrict__ ws /* [cs][T][WS_ROW(N)], tiled */, int T, int ncs, float* __restrict__ ov /* [cs][T][OV_ROW(N)] */ LC3_RAGGED_OPT)
{
    __shared__ Imd4Lds L;
    const int lane = threadIdx.x;
    const int runs = (T + F4_FR - 1) / F4_FR;
    const int cs = blockIdx.x / runs, t0 = (blockIdx.x % runs) * F4_FR;
    if (cs >= ncs) return;
    const int nf = imin(F4_FR, DEC_TC(cs / P->channels) - t0);
#ifdef LC3_DEC_RAGGED
    if (nf <= 0) return;                              /* a group wholly past the stream's count (lc3_dec_kernels.inc: DEC_TC); one that straddles it holds nf frames */
#endif
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    constexpr int N = F4_N, wsr = WS_ROW(F4_N), ovr = OV_ROW_STD;
    const size_t cf0 = (size_t)cs * T + t0;
#pragma unroll
    for (int f = 0; f < F4_FR; f++) {
        const int ff = f < nf ? f : 0;
        L.isc[f][lane] = rec[(cf0 + ff) * PR_WORDS + lane];
        L.gi[f][lane] = __int_as_float(rec[(cf0 + ff) * PR_WORDS + PR_GAINS + lane]);
    }
    LSYNC();
    const int Lspec = DPI(ylen);
    {
        const int nb = DPI(nbands), lim = lc3t_band_pool[DPI(band_off) + nb];
        for (int j = lane; j < N; j += WAVE) { const int b = (int)P->band_of_bin[j]; L.bsel[j] = (unsigned char)((b < nb && j < lim) ? b : 255); }
    }
    LSYNC();
    /* ---- SNS shaping R/mdct_shaping.c: the frames' rows, 16 bytes per lane, times the band gains -> A_f ---- */
    for (int idx = lane; idx < F4_FR * (N / 4); idx += WAVE) {          /* the same chunk of the four frames is 256 consecutive bytes of the tiled rows */
        const int f = (idx >> 2) & 3, j = 16 * (idx >> 4) + 4 * (idx & 3);
        if (f < nf) {
            float4 v = j < Lspec ? *(const float4*)&LC3D_ROW_BASE(ws, cs, t0 + f, T, wsr)[LC3D_ROW_OFF(j, T)] : make_float4(0, 0, 0, 0);
            float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int u = 0; u < 4; u++) { const int b = L.bsel[j + u]; float w = j + u < Lspec ? e[u] : 0.0f; if (b != 255) w = w * L.gi[f][b]; e[u] = w; }
            *(float4*)&L.x[N * f + j] = make_float4(e[0], e[1], e[2], e[3]);
        }
    }
    LSYNC();
    /* ---- lost frames: concealment R/plc_noise_substitution0.c (the last good spectrum with random signs, fading), frame by frame ---- */
    for (int f = 0; f < nf; f++) {
        if (uni(L.isc[f][PR_BFI]) != 1) continue;
        const int src = uni(L.isc[f][PR_PLC + 3]);
        const float ca = __int_as_float(uni(L.isc[f][PR_PLC + 1]));
        int seed = uni(L.isc[f][PR_PLC + 2]);
        constexpr int NRL = (F4_N + 63) / 64;
        float prev[NRL];
        if (src >= 0) {                               /* rebuilt from the hand-over of that frame: same products as when it was decoded */
            const float* rowg = LC3D_ROW_BASE(ws, cs, src, T, wsr);
            LSYNC();
            L.gi[f][lane] = __int_as_float(rec[((size_t)cs * T + src) * PR_WORDS + PR_GAINS + lane]);
            LSYNC();
#pragma unroll
            for (int k = 0; k < NRL; k++) {
                const int j = lane + WAVE * k;
                float v = j < Lspec ? rowg[LC3D_ROW_OFF(j, T)] : 0.0f;
                const int b = j < N ? (int)L.bsel[j] : 255;
                if (b != 255) v = v * L.gi[f][b];
                prev[k] = v;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NRL; k++) { const int j = lane + WAVE * k; prev[k] = j < Lspec ? state[(size_t)cs * DST_WORDS + DST_QPREV + j] : 0.0f; }
        }
#pragma unroll
        for (int k = 0; k < NRL; k++) {
            const int i0 = WAVE * k;
            float mine = 0;
            if (i0 < Lspec) {
                const int cnt = imin(WAVE, Lspec - i0);
                for (int j = 0; j < cnt; j++) {
                    seed = 16831 + seed * 12821;
                    seed = (int)((double)seed - round((double)((float)seed * 0x1p-16f)) * (double)0x1p16f);
                    if (seed == 32768) seed -= 32768;
                    if (lane == j) mine = seed < 0 ? -ca : ca;
                }
            }
            if (i0 + lane < N) L.x[N * f + i0 + lane] = i0 + lane < Lspec ? prev[k] * mine : 0.0f;
        }
        LSYNC();
    }
    /* ---- pre-twiddle R/dct4.c:84-86: A_f -> registers -> Z_f[col][l] (col = i mod 15, l = i mod 16) ---- */
    float zr[4][F4_FR], zi[4][F4_FR];
    if (lane < 60) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = lane + 60 * k;
            const float2 tw = *(const float2*)&P->tw1[2 * i];
#pragma unroll
            for (int f = 0; f < F4_FR; f++) {
                const float ar = L.x[N * f + 2 * i], ai = L.x[N * f + N - 2 * i - 1];
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
    f4_dft240x4(L.x, P, DPF(dct4_norm), lane);
    /* ---- the time-domain aliasing buffers -> HBM (the synthesis kernel reads them through the fold pattern of R/imdct.c:34-58) ---- */
    for (int idx = lane; idx < F4_FR * (N / 4); idx += WAVE) {
        const int f = idx / (N / 4), q = idx - f * (N / 4);
        if (f < nf) *(float4*)&ov[(cf0 + f) * ovr + 4 * q] = *(const float4*)&L.x[N * f + 4 * q];
    }
}
