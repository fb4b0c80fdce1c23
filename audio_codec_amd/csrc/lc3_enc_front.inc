/* lc3_enc_front.inc -- the stateless front of the encoder, frame-parallel (included by lc3_kernels.hip).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  Low-delay MDCT (R/mdct.c:103-124), per-band energies
 * (R/per_band_energy.c), bandwidth detector (R/detect_cutoff_warped.c) and the SNS scale factors (R/sns_compute_scf.c) of a frame need
 * that frame's PCM and the tail of the previous frame's - nothing the encoder carries from frame to frame.  (The attack detector's
 * block energies are computed here too; its frame-to-frame decision is lc3_enc_attack_kernel below, one stream per lane, and the
 * smoothing it asks for is applied by the vector quantiser's kernel.)  So they run for all B x T frames
 * of a launch at once, a run of `fpw` consecutive frames per wave (the MDCT memory then slides inside LDS as in the sequential
 * kernel; one frame per wave where the launch is a short run of the pipelined path and its latency counts), with the stage functions of lc3_kernels.hip unchanged; the sequential kernel picks the spectrum and the record up from HBM.
 * The wave that owns a stream's last frame hands the MDCT memory for the next launch to the sequential kernel, which stores it in the
 * stream's state (waves of this kernel that start a stream's launch are still reading that state).
 *
 * FRONT_PCM_FMT 0: everything, the kernel for the reference's three PCM formats (16, 24, 32 in the default layout) token for token what it was before the PCM
 * format word existed.  FRONT_PCM_FMT 1 (the -DLC3_PCM_FMT objects): the front kernel alone, named with _fmt, for the formats beyond those (float samples, the
 * interleaved and the channel-major layout, lc3_plan.h: lc3d_pcm_*); the two differ in the PCM load alone. */
#ifndef FRONT_WAVES
#ifdef LC3_BIG
#define FRONT_WAVES 2
#else
#define FRONT_WAVES 5
#endif
#endif
#undef FRONT_KERNEL_NAME
#if defined(LC3_BIG) && FRONT_PCM_FMT
#define FRONT_KERNEL_NAME LC3_FMT_CAT(lc3_enc_front_kernel_big)
#elif defined(LC3_BIG)
#define FRONT_KERNEL_NAME lc3_enc_front_kernel_big
#elif FRONT_PCM_FMT
#define FRONT_KERNEL_NAME ERP_FN(LC3_FMT_CAT(lc3_enc_front_kernel))
#else
#define FRONT_KERNEL_NAME ERP_FN(lc3_enc_front_kernel)
#endif

extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(FRONT_WAVES, FRONT_WAVES)))
FRONT_KERNEL_NAME(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, const float* __restrict__ state, const void* __restrict__ pcm, int bitdepth,
                     int T, int tb, int nt /* frames tb ... tb + nt - 1 of the call's T */, int fpw /* consecutive frames per wave */, int ncs, float* __restrict__ spec /* [cs][RT][srow]: the first ylen lines (the coded ones); frame t of this launch is row r0 + t */, int srow, int RT, int r0, float* __restrict__ rec /* [cs][RT][FR_WORDS] */,
                     float* __restrict__ xnext /* [cs][MEMCAP]: the MDCT memory after the last frame (the sequential kernel moves it into the state) */,
                     const float* __restrict__ xprev /* the MDCT memory before frame 0: the state's slot, or the previous call's xnext */, int xprev_stride,
                     int do_scf /* band energies, bandwidth detector and scale factors here (0: lc3_enc_scf_lane_kernel does them, one frame per lane) */ LC3_PLACED_OPT LC3_ERP_OPT)
{
    __shared__ FrontLds L;
    const int lane = threadIdx.x;
    const int runs = (nt + fpw - 1) / fpw;
#ifdef LC3_ENC_RPIPE                /* ragged: the run ends at the stream's count tend, and the wave that holds frame tend - 1 hands the MDCT memory over */
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * fpw;
    if (cs >= ncs) return;
    const int tend = cnt[cs / P->channels], t1 = imin(imin(tb + nt, t0 + fpw), tend);
    if (t0 >= t1) return;
#else
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * fpw, t1 = imin(tb + nt, t0 + fpw), tend = T;
    if (cs >= ncs) return;
#endif
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    if (lane < 14) L.cc[lane] = ((const int*)&chans[cs])[lane];
    if (lane < 56) L.isc[lane] = 0;                                        /* I_ATT_FLAG = 0: the smoothing is applied later (lc3_enc_snsvq_kernel) */
    LSYNC();
    const int N = PI(N), channels = PI(channels), ml = N - PI(la);
    const int strm = cs / channels, ch = cs - strm * channels;
    const float* stp = state + (size_t)cs * LC3D_STATE_WORDS(MEMCAP);
    const float sc = bitdepth == 24 ? 256.0f : 65536.0f;
    /* MDCT memory = the last N - la_zeros samples of the frame before the run (R/mdct.c:111), right-aligned in its slot */
    if (t0 == 0) { for (int i = lane; i < MEMCAP; i += WAVE) L.xbuf[i] = xprev[(size_t)cs * xprev_stride + i]; }
#ifdef LC3_PCM_PLACED
    else pcm_placed_load<false>(pcm, bitdepth, plo, plcap, channels, N, (size_t)strm * T + t0 - 1, ch, N - ml, ml, &L.xbuf[MEMCAP - ml], lane, 1.0f);
#elif FRONT_PCM_FMT
    else {
        const int ps = lc3d_pcm_stride(bitdepth, channels);
        const size_t pidx = lc3d_pcm_frame(bitdepth, channels, T, N, strm, t0 - 1, ch) + (size_t)(N - ml) * ps;
        for (int j = lane; j < ml; j += WAVE) L.xbuf[MEMCAP - ml + j] = PCM_IN(pcm, bitdepth, pidx + (size_t)j * ps);
    }
#else
    else {
        const size_t pidx = (((size_t)strm * T + t0 - 1) * channels + ch) * N + (N - ml);
        for (int j = lane; j < ml; j += WAVE)
            L.xbuf[MEMCAP - ml + j] = bitdepth == 16 ? (float)((const int16_t*)pcm)[pidx + j] : (float)((const int32_t*)pcm)[pidx + j] / sc;
    }
#endif
    /* attack detector, first half (R/attack_detector.c:26-77): its filter memory entering a frame is the last two 16 kHz samples of the
     * previous frame - the state for the first frame of a launch, a function of the previous frame's PCM otherwise */
    const bool att = CI(attack_handling) != 0;
    float am0 = 0, am1 = 0;
    if (att) {
        if (t0 == 0) { if (!CI(reset_attack)) { am0 = stp[LC3D_ST_SCAL(MEMCAP) + F_ATT_M0]; am1 = stp[LC3D_ST_SCAL(MEMCAP) + F_ATT_M1]; } }
        else {
            LSYNC();
            const float* q = &L.xbuf[MEMCAP];        /* one past the previous frame's last sample */
            if (PI(fs) == 96000) { am0 = q[-12] + q[-11] + q[-10] + q[-9] + q[-8] + q[-7]; am1 = q[-6] + q[-5] + q[-4] + q[-3] + q[-2] + q[-1]; }
            else if (PI(fs) == 48000) { am0 = (q[-6] + q[-5] + q[-4]); am1 = (q[-3] + q[-2] + q[-1]); }
            else if (PI(fs) == 32000) { am0 = (q[-4] + q[-3]); am1 = (q[-2] + q[-1]); }
            else { am0 = (float)((double)q[-6] + ((double)(q[-5] + q[-4])) / 2.0); am1 = (float)((double)q[-3] + ((double)(q[-2] + q[-1])) / 2.0); }
        }
    }
    for (int t = t0; t < t1; t++) {
#ifdef LC3_PCM_PLACED
        pcm_placed_load<true>(pcm, bitdepth, plo, plcap, channels, N, (size_t)strm * T + t, ch, 0, N, XCUR(L), lane, 1.0f);
#elif FRONT_PCM_FMT
        {                                                                              /* by the format word: the frame's first element and the step between its samples */
            const size_t o = lc3d_pcm_frame(bitdepth, channels, T, N, strm, t, ch);
            if (PCM_F32_WIDE(pcm, bitdepth, o, N)) {                                   /* float samples one after the other: 16 bytes per lane */
                const float4* p = (const float4*)((const float*)pcm + o);
                for (int i = lane; i < (N >> 2); i += WAVE) *(float4*)&XCUR(L)[4 * i] = pcm_f32x4(p[i]);
            } else {
                const int ps = lc3d_pcm_stride(bitdepth, channels);
                for (int i = PCM_RUN(true, pcm, bitdepth, o, N, XCUR(L), lane, 1.0f) + lane; i < N; i += WAVE) XCUR(L)[i] = PCM_IN(pcm, bitdepth, o + (size_t)i * ps);
            }
        }
#else
        const size_t fidx = ((size_t)strm * T + t) * channels + ch;
        if (bitdepth == 16) {
            const int16_t* p = (const int16_t*)pcm + fidx * N;
            if ((N & 7) == 0 && (((size_t)p) & 15) == 0) {
                for (int i = lane; i < (N >> 3); i += WAVE) {
                    const uint4 v = ((const uint4*)p)[i];
                    float* d = &XCUR(L)[8 * i];
                    d[0] = (float)(int16_t)(v.x & 0xffff); d[1] = (float)(int16_t)(v.x >> 16);
                    d[2] = (float)(int16_t)(v.y & 0xffff); d[3] = (float)(int16_t)(v.y >> 16);
                    d[4] = (float)(int16_t)(v.z & 0xffff); d[5] = (float)(int16_t)(v.z >> 16);
                    d[6] = (float)(int16_t)(v.w & 0xffff); d[7] = (float)(int16_t)(v.w >> 16);
                }
            } else for (int i = lane; i < N; i += WAVE) XCUR(L)[i] = (float)p[i];
        } else {
            const int32_t* p = (const int32_t*)pcm + fidx * N;
            for (int i = lane; i < N; i += WAVE) XCUR(L)[i] = (float)p[i] / sc;
        }
#endif
        LSYNC();
        float* r = rec + ((size_t)cs * RT + r0 + t) * FR_WORDS;
        if (att) {
            float n0, n1;
            const float e = attack_energies(L, lane, am0, am1, n0, n1);
            if (lane < 4) r[FR_ATT + lane] = lane < PI(att_nblocks) ? e : 0.0f;
            if (lane == 0) { r[FR_ATTM] = n0; r[FR_ATTM + 1] = n1; }
            am0 = n0; am1 = n1;
            LSYNC();
        }
        mdct_pre(P, L, lane);
#ifdef LC3_BIG
        if (PI(N) == 960) { mdct_dft480_cols(L, lane); mdct_dft480_rows(L, lane); } else
#endif
        if (PI(N) == 480) { mdct_dft240_cols(L, lane); mdct_dft240_rows(L, lane); }
        else if (PI(N) == 120) mdct_dft60(P, L, lane);
        else { if (PI(N) == 320) mdct_dft160_stage1(P, L, lane); else if (PI(N) == 160) mdct_dft80_stage1(P, L, lane); mdct_dft_pfa(P, L, lane); }
        mdct_post(P, L, lane);
#ifdef DUP_MDCT
        mdct_pre(P, L, lane);
#ifdef LC3_BIG
        if (PI(N) == 960) { mdct_dft480_cols(L, lane); mdct_dft480_rows(L, lane); } else
#endif
        if (PI(N) == 480) { mdct_dft240_cols(L, lane); mdct_dft240_rows(L, lane); }
        else if (PI(N) == 120) mdct_dft60(P, L, lane);
        else { if (PI(N) == 320) mdct_dft160_stage1(P, L, lane); else if (PI(N) == 160) mdct_dft80_stage1(P, L, lane); mdct_dft_pfa(P, L, lane); }
        mdct_post(P, L, lane);
#endif
        float* sp = LC3D_ROW_BASE(spec, cs, r0 + t, RT, srow);
        for (int i = lane; i < PI(ylen); i += WAVE) sp[LC3D_ROW_OFF(i, RT)] = L.A[i];          /* the unshaped spectrum (shaping needs the quantised scale factors); lines from ylen on are never coded */
        if (do_scf) {
            st_energy_bw(P, L, lane);
            LSYNC();
            st_sns_scf(P, L, lane);
            if (lane < 16) r[FR_SCF + lane] = L.sm[SM_SCF + lane];
            if (lane == 0) ((int*)r)[FR_BW] = L.isc[I_BW];
        }
        if (lane == 0) ((int*)r)[FR_ATTFLAG] = 0;   /* lc3_enc_attack_kernel sets the flag where the detector runs */
        LSYNC();
    }
    if (t1 == tend) for (int i = lane; i < MEMCAP; i += WAVE) xnext[(size_t)cs * MEMCAP + i] = L.xbuf[i];
}

#if !defined(LC3_BIG) && !FRONT_PCM_FMT
/* attack detector, second half (R/attack_detector.c:79-102): one channel-stream per lane walks the frames of the launch over the block
 * energies the front kernel left in the records and writes each frame's flag back; the detector's state lives in the stream's state
 * words (same words the sequential kernel uses on its own path).  A pending reset (R/setup_enc_lc3.c:297-308) is applied first. */
extern "C" __global__ void __launch_bounds__(WAVE)
ERP_FN(lc3_enc_attack_kernel)(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, float* __restrict__ state, int state_words, int scal_off,
                      float* __restrict__ rec /* [cs][RT][FR_WORDS], frame t = row r0 + t */, int RT, int r0, int tb, int nt, int ncs LC3_ERP_OPT)
{
    const int cs = blockIdx.x * WAVE + threadIdx.x;
    if (cs >= ncs) return;
    float* sc = state + (size_t)cs * state_words + scal_off; int* isc = (int*)sc + 16;
#ifdef LC3_ENC_RPIPE                /* ragged: the stream's present frames of this launch (none: nothing at all), the state from the record of the last of them; a pending reset
                                     * belongs to the stream's first present frame - the launch that holds frame 0 - and stays pending for a stream with no frame (the tail kernel) */
    nt = imin(nt, cnt[cs / P->channels] - tb);
    if (nt <= 0) return;
    if (tb == 0 && chans[cs].reset_attack)
#else
    if (chans[cs].reset_attack)
#endif
    { sc[F_ATT_M0] = 0; sc[F_ATT_M1] = 0; sc[F_ATT_ACC] = 0; isc[I_ATT_POS] = 0; isc[I_ATT_FLAG] = 0; }
    if (!chans[cs].attack_handling || nt <= 0) return;
    float acc = sc[F_ATT_ACC]; int pos = isc[I_ATT_POS], flag = 0;
    const int nb = P->att_nblocks, hang = P->att_hang; const float mval = P->fs == 96000 ? 1e-5f : 0.0f;
    float* r = rec + ((size_t)cs * RT + r0 + tb) * FR_WORDS;
    float4 e = *(const float4*)&r[FR_ATT];
    for (int t = 0; t < nt; t++) {
        const float4 en = t + 1 < nt ? *(const float4*)&r[(size_t)(t + 1) * FR_WORDS + FR_ATT] : e;
        attack_decide(e.x, e.y, e.z, e.w, nb, mval, hang, acc, pos, flag);
        ((int*)r)[(size_t)t * FR_WORDS + FR_ATTFLAG] = flag;
        e = en;
    }
    const float* rl = r + (size_t)(nt - 1) * FR_WORDS;
    sc[F_ATT_M0] = rl[FR_ATTM]; sc[F_ATT_M1] = rl[FR_ATTM + 1]; sc[F_ATT_ACC] = acc; isc[I_ATT_POS] = pos; isc[I_ATT_FLAG] = flag;
}
#endif
