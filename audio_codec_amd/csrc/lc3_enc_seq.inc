/* lc3_enc_seq.inc -- the pitch chain of the pipelined encoder path (included by lc3_kernels.hip; the rate chain: lc3_enc_rate.inc).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  What carries state from frame to frame in Enc_LC3_Channel_fl
 * (R/enc_lc3_fl.c:44-132) falls into two independent chains:
 *   pitch chain : OLPA (R/olpa.c) and the LTPF coder (R/ltpf_coder.c) - histories of the 12.8 / 6.4 kHz signal, pitch and LTPF decision
 *                 memories; consumes the HP-filtered 12.8 kHz samples, produces four integers per frame;
 *   rate chain  : SNS shaping, TNS, global-gain estimate, quantisation + bit estimate, gain adjustment, noise level, residual - of these
 *                 only the gain estimate reads what the previous frame left (three rate-control words); consumes the spectrum and the
 *                 record of the frame-parallel front / quantiser kernels plus the pitch chain's four integers.
 * In lc3_encode_kernel one wave runs both for its stream with a 10 KB LDS slice and 128 registers, which fills the chip with exactly
 * one wave per stream.  Here each chain is a kernel with the slice and the registers it needs (pitch: 5 KB / 54 registers, rate:
 * 6.5 KB / 64), one wave per channel-stream each, launched per RUN of frames on different HIP streams: the pitch kernel and the
 * frame-parallel kernels of run k+1 are resident beside the rate kernel of run k, which gives every SIMD six to eight waves to choose
 * from instead of four.  Both use the stage functions of lc3_kernels.hip unchanged (they are templates over the slice type).
 *
 * All buffers are rows of T frames (the frames of the call); a launch covers frames t0 ... t0 + nt - 1. */

/* -DDUP_<STAGE> (tools/dup_profile.sh, diagnostic builds only): the named stage runs twice, so that the difference of the kernel's
 * instruction counters to the plain build is the stage; the output of such a build is not the encoder's. */
#ifndef LC3_BIG
struct __attribute__((aligned(16))) PitchLds {
    static constexpr int MISC = 0;
    static constexpr int XOFF = 0;
    float xbuf[4];              /* unused (the stage functions only name it through XCUR) */
    float A[384];               /* scratch: products of the ordered sums */
    float h12[384];             /* HP-filtered 12.8 kHz stream, newest sample at [383] */
    float h6[194];              /* 6.4 kHz stream, newest at [193] */
    float sm[128];              /* 98 autocorrelations / LTPF correlation tables */
    int   pc[LC3D_PLAN_HEAD_WORDS];
    int   cc[14];
    float fsc[12];
    int   isc[56];
#ifdef LC3_STAGE_TIMING
    long long tacc[NSTAGE];
#endif
};

extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(8, 8)))
ERP_FN(lc3_enc_pitch_kernel)(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, float* __restrict__ state, int state_words, int memcap,
                     const float* __restrict__ y12 /* [cs][T][128] */, int T, int t0, int nt, int ncs, float* __restrict__ frec /* [cs][RT][FR_WORDS], frame t = row r0 + t */, int RT, int r0 LC3_ERP_OPT)
{
#ifdef PITCH_PRIO
    __builtin_amdgcn_s_setprio(PITCH_PRIO);
#endif
    __shared__ PitchLds L;
    const int lane = threadIdx.x, cs = blockIdx.x;
    if (cs >= ncs) return;
#ifdef LC3_ENC_RPIPE                /* ragged: the stream's frames of this launch that are present; none - the stream's histories stay what they are */
    nt = imin(nt, cnt[cs / P->channels] - t0);
    if (nt <= 0) return;
#endif
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    if (lane < 14) L.cc[lane] = ((const int*)&chans[cs])[lane];
    const lc3d_chan* __restrict__ C = &chans[cs];
    float* stp = state + (size_t)cs * state_words;
    for (int i = lane; i < 384; i += WAVE) L.h12[i] = stp[LC3D_ST_H12(memcap) + i];
    for (int i = lane; i < 194; i += WAVE) L.h6[i] = stp[LC3D_ST_H6(memcap) + i];
    if (lane < 12) L.fsc[lane] = stp[LC3D_ST_SCAL(memcap) + lane];
    if (lane < 16) L.isc[lane] = ((const int*)stp)[LC3D_ST_SCAL(memcap) + 16 + lane];
    LSYNC();
    const int len12 = PI(len12);
    float ny0 = 0, ny1 = 0;
    if (nt > 0) { const float* yp = y12 + ((size_t)cs * T + t0) * 128; ny0 = lane < len12 ? yp[lane] : 0.0f; ny1 = lane + 64 < len12 ? yp[lane + 64] : 0.0f; }
    for (int t = t0; t < t0 + nt; t++) {
        const float y0 = ny0, y1 = ny1;
        if (t + 1 < t0 + nt) { const float* yp = y12 + ((size_t)cs * T + t + 1) * 128; ny0 = lane < len12 ? yp[lane] : 0.0f; ny1 = lane + 64 < len12 ? yp[lane + 64] : 0.0f; }
        float keep[6];
#pragma unroll
        for (int k = 0; k < 6; k++) { const int i = lane + 64 * k; keep[k] = (i + len12 < 384) ? L.h12[i + len12] : 0.0f; }
        LSYNC();
#pragma unroll
        for (int k = 0; k < 6; k++) { const int i = lane + 64 * k; if (i + len12 < 384) L.h12[i] = keep[k]; }
        if (lane < len12) L.h12[384 - len12 + lane] = y0;
        if (lane + 64 < len12) L.h12[384 - len12 + 64 + lane] = y1;
        LSYNC();
        st_olpa(P, L, lane);
#ifdef DUP_OLPA
        st_olpa(P, L, lane);
#endif
        st_ltpf(P, C, L, lane);
#ifdef DUP_LTPF
        st_ltpf(P, C, L, lane);
#endif
        if (lane < 4) ((int*)frec)[((size_t)cs * RT + r0 + t) * FR_WORDS + FR_LTPF + lane] = L.isc[I_LTPF0 + lane];     /* flag, active, pitch index, side bits */
        LSYNC();
    }
    for (int i = lane; i < 384; i += WAVE) stp[LC3D_ST_H12(memcap) + i] = L.h12[i];
    for (int i = lane; i < 194; i += WAVE) stp[LC3D_ST_H6(memcap) + i] = L.h6[i];
    if (lane >= F_LTPF_NC1 && lane <= F_LTPF_PITCH) stp[LC3D_ST_SCAL(memcap) + lane] = L.fsc[lane];
    if (lane == I_OLPA_PITCH || lane == I_LTPF_ON) ((int*)stp)[LC3D_ST_SCAL(memcap) + 16 + lane] = L.isc[lane];
}
#endif
