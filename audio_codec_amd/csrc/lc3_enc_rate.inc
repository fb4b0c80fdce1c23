/* lc3_enc_rate.inc -- the rate chain of the pipelined encoder path, cut down to its recurrence (included by lc3_kernels.hip).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  Of everything Enc_LC3_Channel_fl does behind the SNS quantiser
 * (R/enc_lc3_fl.c:95-160) only two lines read what the previous frame left: the global-gain estimate takes the rate loop's
 * (targetBitsOff, mem_targetBits, mem_specBits) (R/estimate_global_gain.c:42-50), and mem_specBits is the bit count of the FIRST
 * quantisation (R/enc_lc3_fl.c:120).  So the frame-to-frame chain is: rate update -> bisection of the gain index against the
 * updated target (:93-137) -> quantisation at that gain and its exact bit count (R/quantize_spec.c:26-170, the estimate only).
 * Everything else is a function of the frame alone and runs for all frames of a run at once:
 *
 *   lc3_enc_shape_kernel  (a run of frames per wave, frames independent; behind lc3_enc_snsvq_kernel)
 *       SNS interpolation + shaping (R/sns_interpolate_scf.c, R/mdct_shaping.c), bandwidth controller (R/cutoff_bandwidth.c), TNS
 *       (R/tns_coder.c), spectrum maximum / smallest gain index / the 4-bin log energies en[] (R/estimate_global_gain.c:52-91).
 *       Rewrites the frame's spectrum row in place and appends en[]; TNS parameters and the gain floor go to the record.
 *   lc3_enc_rate_kernel   (one channel-stream per wave, frames in order)
 *       the chain above.  The spectrum is read straight into registers in tuple order (a lane owns lines 2p, 2p + 1): no LDS
 *       spectrum, no LDS quantised lines; en[] in registers.  Leaves four words per frame: gain index, gain, bits, lastnz.
 *   lc3_enc_pack_kernel   (one frame per LANE, lc3_enc_pack.inc)
 *       gain adjustment (R/adjust_global_gain.c) and, when it moved the gain, the second quantisation with its truncating bit count
 *       (R/enc_lc3_fl.c:123-132), noise level (R/noise_factor.c), residual bits (R/residual_coding.c) as the reference's own scalar loops
 *       per lane, straight into the bitstream writer.
 *
 * All buffers are rows of T frames (the frames of the call); a launch covers frames t0 ... t0 + nt - 1. */

#ifdef LC3_BIG
#define SHAPE_KERNEL_NAME lc3_enc_shape_kernel_big
#define RATE_KERNEL_NAME  lc3_enc_rate_kernel_big
#define TAILW_KERNEL_NAME lc3_enc_tailw_kernel_big
#define SHAPE_WAVES 3
#ifndef RATE_WAVES_BIG
#define RATE_WAVES_BIG 4        /* 128 registers.  The large layout's kernel keeps twice the per-lane tuple state: under the standard kernel's 96 registers 87 of them went to scratch.
                                * Measured on c96: 5 waves (87 spilled) 37.05, 4 waves (28 spilled) 38.07, 3 waves (165 registers, none spilled) 33.16 Mframes/s */
#endif
#define RATE_WAVES RATE_WAVES_BIG
#else
#ifdef LC3_ENC_VBW
#define SHAPE_KERNEL_NAME lc3_enc_shape_kernel_vbw      /* per-frame bandwidths (lc3_kernels.hip, -DLC3_ENC_VBW): only this kernel of the file */
#else
#define SHAPE_KERNEL_NAME lc3_enc_shape_kernel
#endif
#define RATE_KERNEL_NAME  ERP_FN(lc3_enc_rate_kernel)
#define TAILW_KERNEL_NAME lc3_enc_tailw_kernel
#ifndef SHAPE_WAVES
#define SHAPE_WAVES 4          /* 128 registers: under a smaller budget the TNS functions spill (measured: 6 waves 50.6, 5: 52.6, 4: 65.3, 3: 65.2 Mframes/s) */
#endif
#ifndef RATE_WAVES
#define RATE_WAVES 5          /* 96 registers: no spills (a scratch reload is counted with the vector loads and would wait for the prefetch) */
#endif
#endif

#ifndef LC3_ENC_RPIPE       /* (the ragged object takes the rate kernel alone: the wave-per-frame shape kernel and the frame-per-wave writer are diagnostic variants without ragged forms) */
/* ------------------------------------------------------------------------------------------------------------------------------ */
struct __attribute__((aligned(16))) ShapeLds {
    static constexpr int MISC = 0;
    static constexpr int XOFF = 0;
    static constexpr int TNS0 = 96, TNS1 = 96 + 184;   /* behind the 64 interpolated gains and the 16 quantised scale factors (SM_SCFQ = 80) */
    float xbuf[MAXN];           /* the parked spectrum, then the TNS lattice's output */
    float A[MAXN];              /* the spectrum (shaped / TNS-filtered in place) */
    float sm[96 + 184 + 80];
    int   pc[LC3D_PLAN_HEAD_WORDS];
    int   cc[14];
    float fsc[12];
    int   isc[56];
#ifdef LC3_STAGE_TIMING
    long long tacc[NSTAGE];
#endif
};

extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(SHAPE_WAVES, SHAPE_WAVES)))
SHAPE_KERNEL_NAME(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int T /* rows per channel-stream */, int tb, int nt, int fpw, int ncs,
                  float* __restrict__ rows /* [cs][T][srow] */, int srow, float* __restrict__ frec /* [cs][T][FR_WORDS] */
#ifdef LC3_ENC_VBW
                  , const uint16_t* __restrict__ bwf /* [stream][T] bandwidth in force for each stream-frame, Hz */
#endif
                  )
{
    __shared__ ShapeLds L;
    const int lane = threadIdx.x;
    const int runs = (nt + fpw - 1) / fpw;
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * fpw, t1 = imin(tb + nt, t0 + fpw);
    if (cs >= ncs) return;
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    if (lane < 14) L.cc[lane] = ((const int*)&chans[cs])[lane];
    if (lane < 56) L.isc[lane] = 0;
    LSYNC();
    const lc3d_chan* __restrict__ C = &chans[cs];
    const int N = PI(N), ylen = PI(ylen);
    constexpr int SPK = (MAXN + WAVE - 1) / WAVE;
    unsigned bob[4] = {0, 0, 0, 0};                  /* band of this lane's bins, one byte each: the table look-up of the SNS shaping, once per launch */
#pragma unroll
    for (int k = 0; k < SPK; k++) { const int j = lane + 64 * k; bob[k >> 2] |= (unsigned)(j < N ? P->band_of_bin[j] : 255) << (8 * (k & 3)); }
    float sp[SPK]; float rq = 0; int rb = 0;
#pragma unroll
    for (int k = 0; k < SPK; k++) sp[k] = 0;
#define SHAPE_PREFETCH(t_) do { const float* sr_ = LC3D_ROW_BASE(rows, cs, (t_), T, srow); const float* fr_ = frec + ((size_t)cs * T + (t_)) * FR_WORDS; \
        _Pragma("unroll") for (int k = 0; k < SPK; k++) sp[k] = lane + 64 * k < ylen ? sr_[LC3D_ROW_OFF(lane + 64 * k, T)] : 0.0f; \
        if (lane < 16) rq = fr_[FR_SCFQ + lane]; \
        if (lane == 0) rb = ((const int*)fr_)[FR_BW]; } while (0)
    SHAPE_PREFETCH(t0);
    for (int t = t0; t < t1; t++) {
        float* row = LC3D_ROW_BASE(rows, cs, t, T, srow);
        float* rec = frec + ((size_t)cs * T + t) * FR_WORDS;
#pragma unroll
        for (int k = 0; k < SPK; k++) if (lane + 64 * k < N) XCUR(L)[lane + 64 * k] = sp[k];      /* lines from ylen on are zero: never coded */
        if (lane < 16) L.sm[SM_SCFQ + lane] = rq;
        if (lane == 0) L.isc[I_BW] = rb;
        LSYNC();
        st_sns_apply(P, L, lane, XCUR(L), bob[0], bob[1], bob[2], bob[3]);
#ifdef DUP_SNSAPPLY
        st_sns_apply(P, L, lane, XCUR(L), bob[0], bob[1], bob[2], bob[3]);
#endif
        int bw = uni(L.isc[I_BW]);
#ifdef LC3_ENC_VBW
        const int fbw = bwf[(size_t)(cs / PI(channels)) * T + t];
        if (fbw) {                                            /* R/cutoff_bandwidth.c:13-26 */
            const int bin = lc3d_bw_cut_bin(fbw, PI(dms));
            if (ylen > bin) {
                if (lane < 4) { const float sc4[4] = {0.5f, 0.25f, 0.125f, 0.0625f}; L.A[bin - 1 + lane] = L.A[bin - 1 + lane] * sc4[lane]; }
                for (int i = bin + 3 + lane; i < ylen; i += WAVE) L.A[i] = 0;
            }
            bw = imin(bw, lc3d_bw_index(fbw));
        }
#else
        if (CI(bandwidth)) {                                  /* R/cutoff_bandwidth.c:13-26 */
            const int bin = CI(bw_cut_bin);
            if (ylen > bin) {
                if (lane < 4) { const float sc4[4] = {0.5f, 0.25f, 0.125f, 0.0625f}; L.A[bin - 1 + lane] = L.A[bin - 1 + lane] * sc4[lane]; }
                for (int i = bin + 3 + lane; i < ylen; i += WAVE) L.A[i] = 0;
            }
            bw = imin(bw, CI(bw_index));
        }
#endif
        const int bw_bin = lc3t_bw_bins[PI(bw_cls) * 6 + bw];
        if (lane < 16) L.isc[I_TNS_IDX0 + lane] = 0;
        if (lane < 2) L.isc[I_TNS_ORD0 + lane] = 0;
        LSYNC();
        st_tns(P, L, lane, bw, bw_bin);
#ifdef DUP_TNS
        st_tns(P, L, lane, bw, bw_bin);
#endif
        st_gain_prep(P, C, L, lane, row, ylen, T, rec);
#ifdef DUP_GAINPREP
        st_gain_prep(P, C, L, lane, row, ylen, T, rec);
#endif
        if (t + 1 < t1) SHAPE_PREFETCH(t + 1);         /* requested here, parked at the top of the next round: nothing lives across the stage calls */
        for (int i = lane; i < ylen; i += WAVE) row[LC3D_ROW_OFF(i, T)] = L.A[i];
        if (lane < 20) ((int*)rec)[FR_TNS + lane] = L.isc[I_TNS_NF + lane];
        if (lane == 0) ((int*)rec)[FR_BWC] = bw;
        LSYNC();
    }
#undef SHAPE_PREFETCH
}
#endif  /* !LC3_ENC_RPIPE */
#ifndef LC3_ENC_VBW

/* ------------------------------------------------------------------------------------------------------------------------------ */
/* The bit-count tables live in LDS, shared by the RATE_WG waves (channel-streams) of a workgroup: a gather from global memory would be waited for with
 * vmcnt, which counts in issue order - the wait would also be for the next frame's spectrum row, requested a frame ahead precisely so that nobody waits
 * for it (measured before: 4 750 of the kernel's 6 200 wave-cycles per frame waiting). */
struct __attribute__((aligned(16))) RateLds {
    uint2    esc[1024];
    uint32_t lut4[1024];
    uint16_t bits[1088];
    int   pc[LC3D_PLAN_HEAD_WORDS];
    int   cc[RATE_WG][14];
};

extern "C" __global__ void __launch_bounds__(RATE_WG * WAVE) __attribute__((amdgpu_waves_per_eu(RATE_WAVES, RATE_WAVES)))
RATE_KERNEL_NAME(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, float* __restrict__ state, int T, int t0, int nt, int ncs,
                 const float* __restrict__ rows /* [cs][T][srow]: shaped spectrum | en[] */, int srow, float* __restrict__ frec /* [cs][T][FR_WORDS] */,
                 const float* __restrict__ xnext /* [cs][MEMCAP]: stored into the state behind the launch's last frame */, int last LC3_ERP_OPT)
{
#ifdef RATE_PRIO
    __builtin_amdgcn_s_setprio(RATE_PRIO);
#endif
    __shared__ RateLds LL;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, cs = blockIdx.x * RATE_WG + wv;
    for (int i = tid; i < 1024; i += RATE_WG * WAVE) { LL.esc[i] = ((const uint2*)P->q_esc)[i]; LL.lut4[i] = P->q_lut4[i]; }
    for (int i = tid; i < 1088 / 2; i += RATE_WG * WAVE) ((uint32_t*)LL.bits)[i] = ((const uint32_t*)P->q_bits)[i];
    if (tid < LC3D_PLAN_HEAD_WORDS) LL.pc[tid] = ((const int*)P)[tid];
    if (lane < 14 && cs < ncs) LL.cc[wv][lane] = ((const int*)&chans[cs])[lane];
    LSYNC();
    if (cs >= ncs) return;
#ifdef LC3_ENC_RPIPE                /* ragged: the stream's present frames of this launch; a stream with no frame in the call is left alone - the hand-over buffer holds another call's data */
    { const int c = cnt[cs / P->channels]; if (c == 0) return; nt = imax(imin(nt, c - t0), 0); }
#endif
    struct { const int* pc; const int* cc; } L = { LL.pc, LL.cc[wv] };      /* what PI() / CI() name */
    float* stp = state + (size_t)cs * LC3D_STATE_WORDS(MEMCAP);
    /* the three words of the rate loop (R/setup_enc_lc3.h: targetBitsOff, mem_targetBits, mem_specBits), wave-uniform */
    float tbits_off = unif(stp[LC3D_ST_SCAL(MEMCAP) + F_TBITS_OFF]);
    int mem_target = uni(((const int*)stp)[LC3D_ST_SCAL(MEMCAP) + 16 + I_MEM_TARGET]), mem_spec = uni(((const int*)stp)[LC3D_ST_SCAL(MEMCAP) + 16 + I_MEM_SPEC]);
    const int ylen = PI(ylen), nq = ylen >> 2, half = ylen >> 1, off = CI(gg_off), fs = PI(fs), tb = CI(total_bits);
    const float offs = PI(hrmode) ? 0.5f : 0.375f;
    int rate = 0;
    if ((fs < 48000 && tb > 320 + (fs / 8000 - 2) * 160) || (fs == 48000 && tb > 800)) rate = 512;
    const float thr7 = PF(c_thr7_up), thr50 = PF(c_thr50_dn);
    const float c_lo_f = (float)((2.7) * (28.0 / 20.0));
    const uint32_t* qlut = LL.lut4; const uint2* qesc = LL.esc; const uint16_t* qbits = LL.bits;
    constexpr int NP = (MAXN / 2 + WAVE - 1) / WAVE;
    float2 nx[NP]; float nev[NQL]; int nr = 0; float ng = 0;
#pragma unroll
    for (int k = 0; k < NP; k++) nx[k] = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int h = 0; h < NQL; h++) nev[h] = 0;
    /* the next frame's row and record words wait in registers while the current frame is worked on */
    /* Every load unconditional, from a clamped in-row address, the masks applied where the values are used: a `cond ? load : 0` is a select on the loaded
     * register, which the compiler can only form behind a wait for the load - seven serialised round trips per frame instead of one overlapped with the frame before */
#define RATE_PREFETCH(t_) do { const float* sr_ = LC3D_ROW_BASE(rows, cs, (t_), T, srow); const float* fr_ = frec + ((size_t)cs * T + (t_)) * FR_WORDS; \
        _Pragma("unroll") for (int k = 0; k < NP; k++) nx[k] = *(const float2*)&sr_[LC3D_ROW_OFF(2 * imin(lane + 64 * k, half - 1), T)]; \
        _Pragma("unroll") for (int h = 0; h < NQL; h++) nev[h] = sr_[LC3D_ROW_OFF(ylen + imin(lane + 64 * h, nq - 1), T)]; \
        nr = ((const int*)fr_)[lane == 0 ? FR_TNS + 3 : lane == 1 ? FR_LTPF + 3 : FR_XZERO]; \
        ng = fr_[FR_GGMIN]; } while (0)
    if (nt > 0) RATE_PREFETCH(t0);
    for (int t = t0; t < t0 + nt; t++) {
        float2 xv[NP]; float ev[NQL];
#pragma unroll
        for (int k = 0; k < NP; k++) xv[k] = lane + 64 * k < half ? nx[k] : make_float2(0.0f, 0.0f);
#pragma unroll
        for (int h = 0; h < NQL; h++) ev[h] = lane + 64 * h < nq ? nev[h] : 0.0f;
        const int tns_bits = __builtin_amdgcn_readlane(nr, 0), ltpf_bits = __builtin_amdgcn_readlane(nr, 1), xzero = __builtin_amdgcn_readlane(nr, 2);
        const float ind_min = unif(ng);
        const float* en = LC3D_ROW_BASE(rows, cs, t, T, srow);
        float* rec = frec + ((size_t)cs * T + t) * FR_WORDS;
        if (t + 1 < t0 + nt) RATE_PREFETCH(t + 1);
        const int tbq = CI(target_bits_init) - (tns_bits + ltpf_bits);
        /* ---- rate loop, R/estimate_global_gain.c:42-50 ---- */
        if (mem_target < 0) tbits_off = 0;
        else {
            float v = tbits_off + (float)mem_target - (float)mem_spec;
            v = -40 > v ? -40 : v; v = 40 < v ? 40 : v;
            tbits_off = (float)(0.8 * (double)tbits_off + 0.2 * (double)v);
        }
        mem_target = tbq;
        const int nbitsSQ = (int)((double)tbq + round((double)tbits_off));
        /* ---- bisection, R/estimate_global_gain.c:93-137 (see st_gain_estimate for the bracketing argument) ---- */
        float ind = 0;
        if (xzero) mem_target = -1;
        else {
            const float target = (float)((28.0 / 20.0) * (1.4) * (double)nbitsSQ);
            const int offset0 = 255 + off;
            int m = 0;
            for (int i = 0; i < 8; i++) {
                const int fac = 128 >> i, cand = offset0 - m - fac;
                const float fc = (float)cand;
                float tsum = 0; int top = -1;
                bool lo_[NQL]; float tv[NQL];
#pragma unroll
                for (int h = NQL - 1; h >= 0; h--) {
                    const bool valid = lane + 64 * h < nq;
                    const float tt = ev[h] - fc;
                    lo_[h] = !valid || tt < thr7;
                    tv[h] = tt > thr50 ? (tt + tt) - 70.0f : tt;
                    const unsigned long long nz = __ballot(!lo_[h]);
                    if (nz && top < 0) top = 64 * h + 63 - (int)__clzll((long long)nz);
                }
#pragma unroll
                for (int h = 0; h < NQL; h++) tsum += lo_[h] ? (lane + 64 * h < top ? c_lo_f : 0.0f) : tv[h];
                const float S = wave_sum_f_tree(tsum);
                bool addback;
                if (top < 0) addback = false;
                else {
                    const float margin = 4e-5f * S + 1e-4f;
                    if (S - margin > target) addback = true;
                    else if (S + margin < target) addback = false;
                    else addback = gain_probe(thr7, thr50, en, ylen, T, nq, cand, target);         /* too close to call: the reference's serial sum */
                }
                if (!addback) m += fac;
            }
            const int offset = offset0 - m;
            if ((float)offset < ind_min) mem_target = -1;
            ind = (ind_min > (float)offset ? ind_min : (float)offset) - (float)off;
        }
        const float gain = P->gain_est[uni((int)(ind + (float)off)) + 256];       /* a scalar load: not counted with the vector loads in flight */
        /* ---- first quantisation and its bit count, R/quantize_spec.c:26-170 with mode -1 (no truncation: the total only).  Lane p owns
         *      the 2-tuple (2p, 2p + 1) of each group of 64 tuples ---- */
        const float rgain = 1.0f / gain;
        int q0[NP], q1[NP]; unsigned amb = 0; int lp = 0;
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const float x0 = xv[k].x, x1 = xv[k].y;
            const float v0 = x0 * rgain + copysignf(offs, x0), v1 = x1 * rgain + copysignf(offs, x1);       /* a zero line: +-offset -> 0, as with no offset */
            q0[k] = (int)v0; q1[k] = (int)v1;
            if (fabsf(v0 - rintf(v0)) <= fabsf(v0) * 5e-7f) amb |= 1u << (2 * k);
            if (fabsf(v1 - rintf(v1)) <= fabsf(v1) * 5e-7f) amb |= 2u << (2 * k);
        }
        if (__ballot(amb != 0)) {                  /* a product that close to an integer: the reference's division for that line */
#pragma unroll
            for (int k = 0; k < NP; k++) {
                if ((amb >> (2 * k)) & 1u) { const float x = xv[k].x; q0[k] = (int)truncf(x / gain + copysignf(offs, x)); }
                if ((amb >> (2 * k)) & 2u) { const float x = xv[k].y; q1[k] = (int)truncf(x / gain + copysignf(offs, x)); }
            }
        }
#pragma unroll
        for (int k = 0; k < NP; k++) { const int p = lane + 64 * k; if (p < half && p >= 1 && (q0[k] != 0 || q1[k] != 0)) lp = p; }
        lp = uni(wave_max_i(lp));
        const int lastnz = lp >= 1 ? 2 * lp + 1 : 1;
        const int ntup = (lastnz + 1) >> 1;
        int meta[NP]; unsigned lutw[NP]; uint2 escw[NP]; int ct1 = 0, ct2 = 0;
#pragma unroll
        for (int k = 0; k < NP; k++) {
            meta[k] = 0; lutw[k] = 0; escw[k] = make_uint2(0, 0);
            if (64 * k < ntup) {
                const int p_ = 64 * k + lane; const bool act_ = p_ < ntup;
                const int x0 = act_ ? q0[k] : 0, x1 = act_ ? q1[k] : 0;
                const int a_ = x0 < 0 ? -x0 : x0, b_ = x1 < 0 ? -x1 : x1, mx_ = imax(a_, b_);
                const int nsh = mx_ >= 4 ? ilog2((unsigned)mx_) - 1 : 0;
                const int af_ = a_ >> nsh, bf_ = b_ >> nsh;
                const int lev1 = imin(nsh, 3), s_ = af_ + bf_;
                const int tval_ = lev1 <= 1 ? 1 + (s_ << lev1) : 12 + lev1;
                const int t1_ = dpp_i<DPP_WSHR1>(ct1, tval_), t2_ = dpp_i<DPP_WSHR1>(ct2, t1_);
                ct2 = __builtin_amdgcn_readlane(tval_, 62); ct1 = __builtin_amdgcn_readlane(tval_, 63);
                int tin = 16 * (t2_ & 15) + t1_ + rate; if (2 * p_ > half) tin += 256;
                if (!act_) tin = 0;
                lutw[k] = qlut[tin]; escw[k] = qesc[tin];
                /* nsh | lev1 << 5 | sym << 7 | non-zero values << 11 | act << 17 */
                meta[k] = nsh | (lev1 << 5) | ((af_ + 4 * bf_) << 7) | ((imin(a_, 1) + imin(b_, 1)) << 11) | ((act_ ? 1 : 0) << 17);
            }
        }
        int bsum = 0;
#pragma unroll
        for (int k = 0; k < NP; k++) {
            if (64 * k < ntup) {
                const int m_ = meta[k], nsh = m_ & 31, lev1 = (m_ >> 5) & 3, sym = (m_ >> 7) & 15;
                const int pkf = (int)((lutw[k] >> (8 * lev1)) & 255u);
                const int bsym = qbits[pkf * 17 + sym];
                const unsigned w_ = nsh >= 3 ? escw[k].y : escw[k].x;
                const int cv = (int)(nsh == 2 ? w_ >> 16 : w_ & 0xffffu), e3 = (int)(escw[k].y >> 16);
                int bits = nsh == 0 ? 0 : cv + e3 * imax(nsh - 3, 0);
                bits += ((m_ >> 11) & 3) * 2048 + 4096 * nsh + bsym;
                bsum += ((m_ >> 17) & 1) ? bits : 0;
            }
        }
        const int nbits0 = (wave_sum_i(bsum) + 2047) >> 11;
        mem_spec = nbits0;                         /* R/enc_lc3_fl.c:120 */
        if (lane < 4) ((int*)rec)[FR_RATE + lane] = lane == 0 ? (int)ind : lane == 1 ? __float_as_int(gain) : lane == 2 ? nbits0 : lastnz;
    }
#undef RATE_PREFETCH
    if (lane == 0) {
        stp[LC3D_ST_SCAL(MEMCAP) + F_TBITS_OFF] = tbits_off;
        ((int*)stp)[LC3D_ST_SCAL(MEMCAP) + 16 + I_MEM_TARGET] = mem_target; ((int*)stp)[LC3D_ST_SCAL(MEMCAP) + 16 + I_MEM_SPEC] = mem_spec;
    }
    /* behind the call's last frame the MDCT memory the front kernel computed goes into the state */
    if (last) for (int i = lane; i < MEMCAP; i += WAVE) stp[LC3D_ST_XPREV + i] = xnext[(size_t)cs * MEMCAP + i];
}


/* ------------------------------------------------------------------------------------------------------------------------------ */
/* TAILW_KERNEL_NAME -- the tail of the encoder and the bitstream writer for LARGE frames, a run of frames per WAVE (frames independent).
 *
 * lc3_enc_pack_kernel codes one frame per lane: its instruction count per frame is the smallest there is, but its duration is the latency of ONE
 * lane coding ONE frame - 0.5 ms at 80 bytes, 1.7 ms at 400 (c5), 3.2 ms at the 320-byte high-resolution frames of c96 - whatever the batch, and it sits
 * at the end of every call.  From a frame size up (lc3hip_opts::tailw_bytes) a frame gets a wave instead: the stage functions of lc3_encode_kernel
 * in its own order (R/enc_lc3_fl.c:113-141) - first quantisation with its bit count (the rate kernel has the same numbers; recomputed here because the
 * wave-parallel writer wants the coder words it leaves), gain adjustment, second quantisation where the gain moved, noise level, residual bits -
 * and st_bitstream, the wave-parallel range coder (64 tuples per step; R/enc_entropy.c, R/ari_codec.c).  More instructions per frame, a fraction of the
 * latency; the two kernels split the streams of a batch by frame size.  MEASURED AND NOT THE DEFAULT (lc3hip_opts::tailw_bytes = 0): byte-identical, but c96
 * 32.5 -> 27.3 and c5 86.5 -> 73.6 Mframes/s with it - the extra instructions cost more than the shorter tail of the call gains.  Kept as a switch
 * (LC3PLUS_ENC_TAILW_BYTES) and as the second user of the stage functions.  in: the shaped, TNS-filtered row and the frame's record; out: the frame's bytes. */
#ifndef LC3_ENC_RPIPE
#ifndef TAILW_WAVES
#define TAILW_WAVES 4
#endif
struct __attribute__((aligned(16))) TailwLds {
    static constexpr bool CDW = true;       /* st_quantize leaves the per-tuple coder words st_bitstream reads */
    static constexpr int MISC = 368;
    static constexpr int XOFF = 0;
    static constexpr int RESO = MAXN / 2, LSTO = MAXN / 2 + 2;
    float xbuf[MAXN];           /* the quantised spectrum */
    float A[MAXN];              /* the shaped, TNS-filtered spectrum; the output frame during the bitstream stage */
    float pad_[2];              /* the list behind the coder words and the residual bits (sm + MAXN / 2 + 2 words) is read in 16-byte pieces */
    float sm[SMW];              /* coder words | residual / LSB bits */
    int   pc[LC3D_PLAN_HEAD_WORDS];
    int   cc[14];
    float fsc[12];
    int   isc[56];
#ifdef LC3_STAGE_TIMING
    long long tacc[NSTAGE];
#endif
};
static_assert(offsetof(TailwLds, A) % 16 == 0 && (offsetof(TailwLds, sm) + (MAXN / 2 + 2) * 4) % 16 == 0, "16-byte aligned LDS rows");

extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(TAILW_WAVES, TAILW_WAVES)))
TAILW_KERNEL_NAME(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int T /* frames of the call = rows per channel-stream */, int nt, int fpw, int ncs,
                  const float* __restrict__ rows /* tiled, lc3_plan.h */, int srow, const float* __restrict__ frec /* [cs][T][FR_WORDS] */,
                  uint8_t* __restrict__ out, int out_stride, uint8_t* __restrict__ status /* [cs][T] */, int min_bytes /* channel-streams below this frame size belong to lc3_enc_pack_kernel */)
{
    __shared__ TailwLds L;
    const int lane = threadIdx.x;
    const int runs = (nt + fpw - 1) / fpw;
    const int cs = blockIdx.x / runs, t0 = (blockIdx.x % runs) * fpw, t1 = imin(nt, t0 + fpw);
    if (cs >= ncs || chans[cs].nbytes < min_bytes) return;
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    if (lane < 14) L.cc[lane] = ((const int*)&chans[cs])[lane];
    if (lane < 56) L.isc[lane] = 0;
    if (lane < 12) L.fsc[lane] = 0;
    LSYNC();
    const lc3d_chan* __restrict__ C = &chans[cs];
    const int ylen = PI(ylen), channels = PI(channels);
    const int strm = cs / channels;
    constexpr int SPK = (MAXN + WAVE - 1) / WAVE;
    float sp[SPK]; int r0 = 0;
#pragma unroll
    for (int k = 0; k < SPK; k++) sp[k] = 0;
    /* record words FR_IDX .. (indices, bandwidth, LTPF, TNS, gain floor, the rate kernel's four) in lanes 0 .. 47 */
#define TAILW_PREFETCH(t_) do { const float* sr_ = LC3D_ROW_BASE(rows, cs, (t_), T, srow); const int* fr_ = (const int*)(frec + ((size_t)cs * T + (t_)) * FR_WORDS); \
        _Pragma("unroll") for (int k = 0; k < SPK; k++) sp[k] = lane + 64 * k < ylen ? sr_[LC3D_ROW_OFF(lane + 64 * k, T)] : 0.0f; \
        r0 = lane < FR_WORDS - FR_IDX ? fr_[FR_IDX + lane] : 0; } while (0)
    TAILW_PREFETCH(t0);
    for (int t = t0; t < t1; t++) {
#pragma unroll
        for (int k = 0; k < SPK; k++) if (lane + 64 * k < MAXN) L.A[lane + 64 * k] = sp[k];
        const int r1 = r0;
        if (lane < 7) L.isc[I_SCF0 + lane] = r1;                                             /* FR_IDX .. */
        if (lane >= FR_LTPF - FR_IDX && lane < FR_LTPF - FR_IDX + 4) L.isc[I_LTPF0 + lane - (FR_LTPF - FR_IDX)] = r1;
        if (lane >= FR_TNS - FR_IDX && lane < FR_TNS - FR_IDX + 20) L.isc[I_TNS_NF + lane - (FR_TNS - FR_IDX)] = r1;
        if (lane == FR_BWC - FR_IDX) L.isc[I_BW] = r1;
        const int gg0 = __builtin_amdgcn_readlane(r1, FR_RATE - FR_IDX);
        const float gain0 = __int_as_float(__builtin_amdgcn_readlane(r1, FR_RATE - FR_IDX + 1));
        const int gg_min = (int)__int_as_float(__builtin_amdgcn_readlane(r1, FR_GGMIN - FR_IDX));
        if (lane == 0) { L.isc[I_GG] = gg0; L.isc[I_GGMIN] = gg_min; L.fsc[F_GAIN] = gain0; }
        if (t + 1 < t1) TAILW_PREFETCH(t + 1);            /* parked in registers across the frame */
        LSYNC();
        const int bw = uni(L.isc[I_BW]);
        const int bw_bin = lc3t_bw_bins[PI(bw_cls) * 6 + bw];
        const int tbq = CI(target_bits_init) - (uni(L.isc[I_TNS_BITS]) + uni(L.isc[I_LTPF_BITS]));
        st_quantize(P, C, L, lane, -1, tbq);
        {
            int gg = gg0, change; float gain = gain0;
            gain_adjust(P, L, gg, gg_min, gain, tbq, uni(L.isc[I_NBITS]), change);               /* R/enc_lc3_fl.c:123-132 */
            LSYNC();
            if (lane == 0) { L.isc[I_GG] = gg; L.fsc[F_GAIN] = gain; L.isc[I_CHANGE] = change; }
            LSYNC();
            if (change) st_quantize(P, C, L, lane, 0, tbq);
        }
        st_noise_factor(P, L, lane, bw_bin);
        if (uni(L.isc[I_LSB]) == 0) st_residual(P, L, lane, tbq, uni(L.isc[I_NBITS2]));
        else { for (int i = lane; i < 160; i += WAVE) ((uint32_t*)RESB(L))[i] = 0; if (lane == 0) L.isc[I_NRES] = 0; LSYNC(); }
        if (!PI(hrmode)) {       /* R/quantize_spec.c:50 asserts that a quantised line fits 16 bits outside the high-resolution mode; here the frame is flagged */
            const int* xq = XQ(L); const int lastnz = uni(L.isc[I_LASTNZ]);
            bool ovf = false;
            for (int i = lane; i < lastnz; i += WAVE) { const int q = xq[i]; ovf |= q != (int)(int16_t)q; }
            if (status && __ballot(ovf) && lane == 0) status[(size_t)cs * T + t] |= LC3D_ENC_ST_QUANT_RANGE;
        }
        st_bitstream(P, C, L, lane);
        LSYNC();
        if (status && lane == 0 && L.isc[I_BUDGET]) status[(size_t)cs * T + t] |= LC3D_ENC_ST_BIT_BUDGET;
        uint8_t* o = out + ((size_t)strm * T + t) * out_stride + CI(out_off);
        const int nby = CI(nbytes);
        if (((nby | (int)(size_t)o) & 3) == 0) { for (int i = lane; i < (nby >> 2); i += WAVE) ((uint32_t*)o)[i] = ((const uint32_t*)BYTES(L))[i]; }
        else for (int i = lane; i < nby; i += WAVE) o[i] = BYTES(L)[i];
        LSYNC();
    }
#undef TAILW_PREFETCH
}
#endif  /* !LC3_ENC_RPIPE */
#endif  /* !LC3_ENC_VBW */
