/* lc3_enc_wave.inc -- the one-wave encode kernel (described in lc3_kernels.hip, which includes this file).
 *
 * ENC_PCM_FMT 0: the kernel KERNEL_FN for the reference's three PCM formats (16, 24, 32 in the default layout), token for token what it was before the PCM format
 * word existed: it sits at its register limit, and any branch more moves its spills.  ENC_PCM_FMT 1 (the -DLC3_PCM_FMT objects): the same kernel named with _fmt
 * for the formats beyond those (float samples, the interleaved and the channel-major layout, lc3_plan.h: lc3d_pcm_*).  The two differ in the PCM load alone.
 * -DLC3_PCM_PLACED: named with _plc, every sample type from per-frame offsets (lc3_kernels.hip: pcm_placed_load).
 * -DLC3_ENC_RAGGED (objects of their own, csrc/Makefile: _erag; the kernels are named with _rag behind _pk, lc3_encode_kernel_var_pk_rag ...): per-stream frame counts (lc3plus_enc_batch_set_frame_counts).  The wave reads its stream's count once
 * (cnt[strm], clamped to 0 ... T by the ragged plan kernel; the channels of a stereo stream share it), returns before it touches anything where that is 0, and runs
 * its frame loop and its one-frame-ahead requests to the count (ENC_TC) instead of T.  T stays the call's frame count: every array is indexed with it.  Without
 * the switch ENC_TC is T, and the kernels are token for token what they were. */
#if ENC_PCM_FMT
#define ENC_WAVE_FN LC3_FMT_CAT(KERNEL_FN)
#else
#define ENC_WAVE_FN KERNEL_FN
#endif
extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(KERNEL_WAVES, KERNEL_WAVES)))
ENC_WAVE_FN(LC3_OW_ARGS LC3_OW_OPT(LC3_OW_ARGS_, LC3_TU_VAR, LC3_TU_VBW, LC3_TU_PK) LC3_PLACED_OPT LC3_ENC_RAGGED_OPT)      /* lc3_kernel_decls.h: the parameters, and what each is */
{
    __shared__ WaveLds L;
    const int lane = threadIdx.x;
    const int cs = blockIdx.x;
    if (cs >= ncs) return;
#ifdef LC3_ENC_RAGGED
    const int Tc = uni(cnt[cs / P->channels]);
    if (Tc <= 0) return;                                 /* nothing of this stream in the call: state, configuration and output stay what they are */
#define ENC_TC Tc
#else
#define ENC_TC T
#endif
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    if (lane < 14) L.cc[lane] = ((const int*)&chans[cs])[lane];
    LSYNC();
    const lc3d_chan* __restrict__ C = &chans[cs];
    const int N = PI(N), channels = PI(channels), ml = N - PI(la);
    const int strm = cs / channels, ch = cs - strm * channels;

    /* ---- load cross-frame state ---- */
    float* stp = state + (size_t)cs * LC3D_STATE_WORDS(MEMCAP);
    for (int i = lane; i < MEMCAP; i += WAVE) L.xbuf[i] = stp[LC3D_ST_XPREV + i];
    for (int i = lane; i < 384; i += WAVE) L.h12[i] = stp[LC3D_ST_H12(MEMCAP) + i];
    for (int i = lane; i < 194; i += WAVE) L.h6[i] = stp[LC3D_ST_H6(MEMCAP) + i];
    if (lane < 12) L.fsc[lane] = stp[LC3D_ST_SCAL(MEMCAP) + lane];
    if (lane < 16) L.isc[lane] = ((const int*)stp)[LC3D_ST_SCAL(MEMCAP) + 16 + lane];
    LSYNC();
    if (CI(reset_attack) && lane == 0) { L.fsc[F_ATT_M0] = 0; L.fsc[F_ATT_M1] = 0; L.fsc[F_ATT_ACC] = 0; L.isc[I_ATT_POS] = 0; L.isc[I_ATT_FLAG] = 0; }
    LSYNC();
#ifdef LC3_STAGE_TIMING
    if (lane < NSTAGE) L.tacc[lane] = 0;
    LSYNC();
    long long tlast = clock64();
#endif

    /* The next frame's PCM (16 bytes per lane when the layout allows) and 12.8 kHz samples are requested one frame ahead and wait
     * in registers: a wave has nothing else to hide a global-memory round trip with at the top of a frame. */
#if !ENC_PCM_FMT
    const bool fast16 = bitdepth == 16 && (N & 7) == 0 && N <= 8 * WAVE && ((((size_t)pcm) + (((size_t)strm * T) * channels + ch) * N * 2) & 15) == 0 && ((N * 2 * channels) & 15) == 0;
    uint4 nv = make_uint4(0, 0, 0, 0);
#endif
    float ny0 = 0, ny1 = 0;
    constexpr int SPK = (MAXN + WAVE - 1) / WAVE;
    unsigned bob[4] = {0, 0, 0, 0};                  /* band of this lane's bins (lane + 64 k), one byte each: the table look-up of the SNS shaping, once per launch */
#pragma unroll
    for (int k = 0; k < SPK; k++) { const int j = lane + 64 * k; bob[k >> 2] |= (unsigned)(j < N ? P->band_of_bin[j] : 255) << (8 * (k & 3)); }
    float sp[SPK]; float rq = 0; int ri = 0;
#pragma unroll
    for (int k = 0; k < SPK; k++) sp[k] = 0;
#define SPEC_PREFETCH(t_) do { const float* sr_ = spec + ((size_t)cs * T + (t_)) * N; const float* fr_ = frec + ((size_t)cs * T + (t_)) * FR_WORDS; \
        _Pragma("unroll") for (int k = 0; k < SPK; k++) sp[k] = lane + 64 * k < N ? sr_[lane + 64 * k] : 0.0f; \
        if (lane < 16) rq = fr_[FR_SCFQ + lane]; \
        if (lane < 8) ri = ((const int*)fr_)[FR_IDX + lane];   /* seven indices, then the bandwidth index */ } while (0)
    if (spec && ENC_TC > 0) SPEC_PREFETCH(0);
    if (ENC_TC > 0) {
#if !ENC_PCM_FMT
        if (fast16 && lane < (N >> 3)) nv = ((const uint4*)((const int16_t*)pcm + (((size_t)strm * T) * channels + ch) * N))[lane];
#endif
        if (y12) { const float* yp = y12 + ((size_t)cs * T) * 128; ny0 = lane < PI(len12) ? yp[lane] : 0.0f; ny1 = lane + 64 < PI(len12) ? yp[lane + 64] : 0.0f; }
    }
    for (int t = 0; t < ENC_TC; t++) {
#ifdef LC3_STAGE_TIMING
        lc3d_trace* tr = nullptr;
#else
        lc3d_trace* tr = trace ? &trace[(size_t)cs * T + t] : nullptr;
#endif
#ifdef LC3_ENC_VAR
        {                                                /* this frame's configuration (the words before out_off) and the channel's payload offset */
            const int fb = fsz[(size_t)strm * dT + dt0 + t];
            const int k = channels == 1 ? fb : ch ? fb >> 1 : (fb + 1) >> 1;
            if (lane < 8) L.cc[lane] = ((const int*)&etab[k])[lane];
            if (lane == 8) L.cc[lane] = ch ? (fb + 1) >> 1 : 0;
            LSYNC();
            if (!CI(attack_handling) && lane == 0) { L.fsc[F_ATT_M0] = 0; L.fsc[F_ATT_M1] = 0; L.fsc[F_ATT_ACC] = 0; L.isc[I_ATT_POS] = 0; L.isc[I_ATT_FLAG] = 0; }
            LSYNC();
        }
#endif
        /* ---- PCM in (R/enc_lc3_fl.c:30-42) ---- */
        const size_t fidx = ((size_t)strm * T + t) * channels + ch;
        /* the frame's spectrum and SNS record from the frame-parallel front were requested at the end of the previous frame: park them in
         * LDS (the frame half of xbuf is free until the quantiser needs it) */
        if (spec) {
#pragma unroll
            for (int k = 0; k < SPK; k++) if (lane + 64 * k < N) XCUR(L)[lane + 64 * k] = sp[k];
            if (lane < 16) L.sm[SM_SCFQ + lane] = rq;
            if (lane < 7) L.isc[I_SCF0 + lane] = ri;
            if (lane == 7) L.isc[I_BW] = ri;
        }
#ifdef LC3_PCM_PLACED                                    /* placed: the frame at its offset, zeros where that is invalid */
        else pcm_placed_load<true>(pcm, bitdepth, plo, plcap, channels, N, (size_t)strm * T + t, ch, 0, N, XCUR(L), lane, 1.0f);
#elif ENC_PCM_FMT
        else {                                           /* by the format word: the frame's first element and the step between its samples */
            const size_t o = lc3d_pcm_frame(bitdepth, channels, T, N, strm, t, ch);
            if (PCM_F32_WIDE(pcm, bitdepth, o, N)) {     /* float samples one after the other: 16 bytes per lane */
                const float4* p = (const float4*)((const float*)pcm + o);
                for (int i = lane; i < (N >> 2); i += WAVE) *(float4*)&XCUR(L)[4 * i] = pcm_f32x4(p[i]);
            } else {
                const int ps = lc3d_pcm_stride(bitdepth, channels);
                for (int i = PCM_RUN(true, pcm, bitdepth, o, N, XCUR(L), lane, 1.0f) + lane; i < N; i += WAVE) XCUR(L)[i] = PCM_IN(pcm, bitdepth, o + (size_t)i * ps);
            }
        }
#else
        else if (fast16) {
            if (lane < (N >> 3)) {
                const uint4 v = nv;
                float* d = &XCUR(L)[8 * lane];
                d[0] = (float)(int16_t)(v.x & 0xffff); d[1] = (float)(int16_t)(v.x >> 16);
                d[2] = (float)(int16_t)(v.y & 0xffff); d[3] = (float)(int16_t)(v.y >> 16);
                d[4] = (float)(int16_t)(v.z & 0xffff); d[5] = (float)(int16_t)(v.z >> 16);
                d[6] = (float)(int16_t)(v.w & 0xffff); d[7] = (float)(int16_t)(v.w >> 16);
            }
            if (t + 1 < ENC_TC && lane < (N >> 3)) nv = ((const uint4*)((const int16_t*)pcm + (fidx + channels) * N))[lane];
        } else if (bitdepth == 16) {
            const int16_t* p = (const int16_t*)pcm + fidx * N;
            for (int i = lane; i < N; i += WAVE) XCUR(L)[i] = (float)p[i];
        } else {
            const int32_t* p = (const int32_t*)pcm + fidx * N;
            const float sc = bitdepth == 24 ? 256.0f : 65536.0f;
            for (int i = lane; i < N; i += WAVE) XCUR(L)[i] = (float)p[i] / sc;
        }
#endif
        LSYNC();
        TICK(0);

        if (y12) {                                       /* lc3_enc_resample_kernel + lc3_enc_hp50_kernel (lc3_enc_pre.inc) have done the work */
            const int len12 = PI(len12);
            const float y0 = ny0, y1 = ny1;
            if (t + 1 < ENC_TC) { const float* yp = y12 + ((size_t)cs * T + t + 1) * 128; ny0 = lane < len12 ? yp[lane] : 0.0f; ny1 = lane + 64 < len12 ? yp[lane + 64] : 0.0f; }
            float keep[6];
#pragma unroll
            for (int k = 0; k < 6; k++) { const int i = lane + 64 * k; keep[k] = (i + len12 < 384) ? L.h12[i + len12] : 0.0f; }
            LSYNC();
#pragma unroll
            for (int k = 0; k < 6; k++) { const int i = lane + 64 * k; if (i + len12 < 384) L.h12[i] = keep[k]; }
            if (lane < len12) L.h12[384 - len12 + lane] = y0;
            if (lane + 64 < len12) L.h12[384 - len12 + 64 + lane] = y1;
            LSYNC();
        } else st_resample(P, L, lane, nullptr);
        TICK(2);
        if (tr) for (int i = lane; i < PI(len12) + 1; i += WAVE) tr->s12k8[i] = L.h12[384 - PI(len12) - 24 + i];
        st_olpa(P, L, lane);
        TICK(3);
        st_ltpf(P, C, L, lane);
        TICK(4);
        if (spec) {
            TICK(5); TICK(1); TICK(6); TICK(7); TICK(8);
        } else {
        if (CI(attack_handling)) st_attack(P, L, lane);
        TICK(5);
        mdct_pre(P, L, lane);
#ifdef LC3_BIG
        if (PI(N) == 960) { mdct_dft480_cols(L, lane); mdct_dft480_rows(L, lane); } else
#endif
        if (PI(N) == 480) { mdct_dft240_cols(L, lane); mdct_dft240_rows(L, lane); }
        else if (PI(N) == 120) mdct_dft60(P, L, lane);
        else { if (PI(N) == 320) mdct_dft160_stage1(P, L, lane); else if (PI(N) == 160) mdct_dft80_stage1(P, L, lane); mdct_dft_pfa(P, L, lane); }
        mdct_post(P, L, lane);
        TICK(1);
        if (tr) for (int i = lane; i < N; i += WAVE) tr->spec_mdct[i] = L.A[i];
        st_energy_bw(P, L, lane);
        TICK(6);
        if (tr) { if (lane == 0) { tr->T0 = L.isc[I_T0]; tr->normcorr = L.fsc[F_NC]; tr->ltpf_param[0] = L.isc[I_LTPF0]; tr->ltpf_param[1] = L.isc[I_LTPF1];
                                   tr->ltpf_param[2] = L.isc[I_LTPF2]; tr->ltpf_bits = L.isc[I_LTPF_BITS]; tr->attack = L.isc[I_ATT_FLAG]; }
                  tr->ener[lane] = lane < PI(nbands) ? L.sm[SM_ENER + lane] : 0; }
        LSYNC();
        st_sns_scf(P, L, lane);
        TICK(7);
        if (tr && lane < 16) tr->scf[lane] = L.sm[SM_SCF + lane];
        st_sns_vq(P, L, lane);
        TICK(8);
        }
        st_sns_apply(P, L, lane, spec ? XCUR(L) : L.A, bob[0], bob[1], bob[2], bob[3]);
        TICK(9);
        if (tr) { if (lane < 16) tr->scf_q[lane] = L.sm[SM_SCFQ + lane]; if (lane < 7) tr->scf_idx[lane] = L.isc[I_SCF0 + lane];
                  for (int i = lane; i < N; i += WAVE) tr->spec_shaped[i] = L.A[i]; }
        int bw = uni(L.isc[I_BW]);
#ifdef LC3_ENC_VBW
        const int fbw = bwf[(size_t)strm * dT + dt0 + t];
        if (fbw) {                                            /* R/cutoff_bandwidth.c:13-26 */
            const int bin = lc3d_bw_cut_bin(fbw, PI(dms));
            if (PI(ylen) > bin) {
                if (lane < 4) { const float sc4[4] = {0.5f, 0.25f, 0.125f, 0.0625f}; L.A[bin - 1 + lane] = L.A[bin - 1 + lane] * sc4[lane]; }
                for (int i = bin + 3 + lane; i < PI(ylen); i += WAVE) L.A[i] = 0;
            }
            bw = imin(bw, lc3d_bw_index(fbw));
            if (lane == 0) L.isc[I_BW] = bw;
        }
#else
        if (CI(bandwidth)) {                                  /* R/cutoff_bandwidth.c:13-26 */
            const int bin = CI(bw_cut_bin);
            if (PI(ylen) > bin) {
                if (lane < 4) { const float sc4[4] = {0.5f, 0.25f, 0.125f, 0.0625f}; L.A[bin - 1 + lane] = L.A[bin - 1 + lane] * sc4[lane]; }
                for (int i = bin + 3 + lane; i < PI(ylen); i += WAVE) L.A[i] = 0;
            }
            bw = imin(bw, CI(bw_index));
            if (lane == 0) L.isc[I_BW] = bw;
        }
#endif
        const int bw_bin = lc3t_bw_bins[PI(bw_cls) * 6 + bw];
        if (lane < 16) L.isc[I_TNS_IDX0 + lane] = 0;
        if (lane < 2) L.isc[I_TNS_ORD0 + lane] = 0;
        LSYNC();
        st_tns(P, L, lane, bw, bw_bin);
        TICK(10);
        const int tns_bits = uni(L.isc[I_TNS_BITS]);
        if (tr) { if (lane == 0) { tr->bw_idx = bw; tr->tns_nfilt = L.isc[I_TNS_NF]; tr->tns_order[0] = L.isc[I_TNS_ORD0]; tr->tns_order[1] = L.isc[I_TNS_ORD1]; tr->tns_bits = tns_bits; }
                  if (lane < 16) tr->tns_rc_idx[lane] = L.isc[I_TNS_IDX0 + lane];
                  for (int i = lane; i < N; i += WAVE) tr->spec_tns[i] = L.A[i]; }
        const int tbq = CI(target_bits_init) - (tns_bits + uni(L.isc[I_LTPF_BITS]));
        st_gain_estimate(P, C, L, lane, tbq);
        TICK(11);
        if (tr && lane == 0) { tr->target_bits_quant = tbq; tr->gain0 = L.fsc[F_GAIN]; tr->gg_idx0 = L.isc[I_GG]; tr->gg_min = L.isc[I_GGMIN]; }
        st_quantize(P, C, L, lane, -1, tbq);
        TICK(12);
        {
            int gg = uni(L.isc[I_GG]), change; float gain = unif(L.fsc[F_GAIN]);
            const int nbits0 = uni(L.isc[I_NBITS]);
            if (tr && lane == 0) tr->nbits0 = nbits0;
            gain_adjust(P, L, gg, uni(L.isc[I_GGMIN]), gain, tbq, nbits0, change);
            LSYNC();
            if (lane == 0) { L.isc[I_MEM_SPEC] = nbits0; L.isc[I_GG] = gg; L.fsc[F_GAIN] = gain; L.isc[I_CHANGE] = change; }
            LSYNC();
            if (change) st_quantize(P, C, L, lane, 0, tbq);
        }
        TICK(13);
        st_noise_factor(P, L, lane, bw_bin);
        TICK(14);
        if (tr) { if (lane == 0) { tr->gain = L.fsc[F_GAIN]; tr->gg_idx = L.isc[I_GG]; tr->gain_change = L.isc[I_CHANGE]; tr->nbits = L.isc[I_NBITS]; tr->nbits2 = L.isc[I_NBITS2];
                                   tr->lastnz = L.isc[I_LASTNZ]; tr->lsb_mode = L.isc[I_LSB]; tr->fac_ns = L.isc[I_FACNS]; }
                  for (int i = lane; i < N; i += WAVE) tr->xq[i] = i < PI(ylen) ? XQ(L)[i] : 0; }
        if (uni(L.isc[I_LSB]) == 0) st_residual(P, L, lane, tbq, uni(L.isc[I_NBITS2]));
        else { for (int i = lane; i < 160; i += WAVE) ((uint32_t*)RESB(L))[i] = 0; if (lane == 0) L.isc[I_NRES] = 0; LSYNC(); }
        TICK(15);
        if (spec && t + 1 < ENC_TC) SPEC_PREFETCH(t + 1);
        if (dump) {
            /* the bitstream of a frame depends on nothing but this: scalars, residual bits, quantised lines up to lastnz.  The
             * serial writer runs one frame per lane in lc3_enc_pack_kernel. */
            int* r = dump + ((size_t)cs * dT + dt0 + t) * dstride;
            if (lane < 56) r[lane] = L.isc[lane];
            const int lastnz = uni(L.isc[I_LASTNZ]), nresw = uni(L.isc[I_LSB]) == 0 ? (uni(L.isc[I_NRES]) + 31) >> 5 : 0;
            for (int i = lane; i < nresw; i += WAVE) r[PK_RES + i] = (int)((const uint32_t*)RESB(L))[i];
            const int* xq = XQ(L);
            if (PI(hrmode)) { for (int i = lane; i < ((lastnz + 1) & ~1); i += WAVE) r[PK_XQ + i] = xq[i]; }
            else {
                /* R/quantize_spec.c:50 asserts that a quantised line fits 16 bits outside the high-resolution mode; here the frame is
                 * flagged instead (the hand-over keeps the low 16 bits) */
                bool ovf = false;
                for (int p = lane; p < ((lastnz + 1) >> 1); p += WAVE) {
                    const int q0 = xq[2 * p], q1 = xq[2 * p + 1];
                    ovf |= q0 != (int)(int16_t)q0 || q1 != (int)(int16_t)q1;
                    r[PK_XQ + p] = (q0 & 0xFFFF) | (q1 << 16);
                }
                if (status && __ballot(ovf) && lane == 0) status[(size_t)cs * dT + dt0 + t] |= LC3D_ENC_ST_QUANT_RANGE;
            }
            LSYNC();
            TICK(16);
            TICK(17);
            continue;
        }
        st_bitstream(P, C, L, lane);
        LSYNC();
        TICK(16);
        if (tr && lane == 0) { tr->n_res_bits = L.isc[I_NRES]; tr->bp_side = L.isc[I_BP_SIDE]; tr->mask_side = L.isc[I_MASK_SIDE]; }
        /* ---- bytes out ---- */
#if defined(LC3_ENC_PACKED)
        const long long po = poff[(size_t)strm * dT + dt0 + t];
        uint8_t* o = out + (po < 0 ? 0 : po) + CI(out_off);
        const int nby = po < 0 ? 0 : CI(nbytes);
#else
#ifdef LC3_ENC_VAR
        uint8_t* o = out + ((size_t)strm * dT + dt0 + t) * out_stride + CI(out_off);
#else
        uint8_t* o = out + ((size_t)strm * T + t) * out_stride + CI(out_off);
#endif
        const int nby = CI(nbytes);
#endif
        if (((nby | (int)(size_t)o) & 3) == 0) { for (int i = lane; i < (nby >> 2); i += WAVE) ((uint32_t*)o)[i] = ((const uint32_t*)BYTES(L))[i]; }
        else for (int i = lane; i < nby; i += WAVE) o[i] = BYTES(L)[i];
        LSYNC();
        TICK(17);
    }
#ifdef LC3_STAGE_TIMING
    if (trace && lane < NSTAGE) ((long long*)&trace[(size_t)cs * T])[lane] = L.tacc[lane];
#endif
    /* ---- store cross-frame state ---- */
    for (int i = lane; i < MEMCAP; i += WAVE) stp[LC3D_ST_XPREV + i] = spec ? xnext[(size_t)cs * MEMCAP + i] : L.xbuf[i];
    for (int i = lane; i < 384; i += WAVE) stp[LC3D_ST_H12(MEMCAP) + i] = L.h12[i];
    for (int i = lane; i < 194; i += WAVE) stp[LC3D_ST_H6(MEMCAP) + i] = L.h6[i];
    /* the HP50 state belongs to lc3_enc_hp50_kernel when it runs, the attack detector's to lc3_enc_attack_kernel on the split path.  Only the scalars that cross a
     * frame are stored (fsc up to F_TBITS_OFF, isc up to I_MEM_SPEC): the ones behind them are every frame's own (F_NC, F_GAIN, I_T0 ..., written before they are read),
     * the pipelined kernels never store them, and get_state() of two batches that encoded the same frames in calls of different shapes must give the same words */
    if (lane <= F_TBITS_OFF && !(y12 && lane < 2) && !(spec && lane >= F_ATT_M0 && lane <= F_ATT_ACC)) stp[LC3D_ST_SCAL(MEMCAP) + lane] = L.fsc[lane];
    if (lane <= I_MEM_SPEC && !(spec && (lane == I_ATT_POS || lane == I_ATT_FLAG))) ((int*)stp)[LC3D_ST_SCAL(MEMCAP) + 16 + lane] = L.isc[lane];
    (void)ml;
}
#undef ENC_TC
