/* lc3_enc_shapel.inc -- SNS shaping, TNS and the stateless half of the gain estimate, one channel-frame per LANE (included by lc3_kernels.hip).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  The same stages as lc3_enc_shape_kernel (lc3_enc_rate.inc) - SNS
 * interpolation (R/sns_interpolate_scf.c:13-89) and shaping (R/mdct_shaping.c:13-22), bandwidth controller (R/cutoff_bandwidth.c:13-26),
 * TNS (R/tns_coder.c:170-362: sub-division autocorrelations, lag window, Levinson-Durbin, LPC weighting, coefficient quantisation, the
 * MA lattice), spectrum maximum, smallest gain index and the 4-bin log energies (R/estimate_global_gain.c:52-91) - but every lane runs
 * the reference's own scalar loops for its frame.  A wave that owns one frame spends most of these stages on short serial chains
 * (Levinson on two lanes, the lattice replaying eight inputs for every four it filters, wave-uniform bookkeeping on the scalar unit):
 * 2 370 instructions per frame; one frame per lane needs about a third of that per frame, with all 64 lanes live.
 *
 * Memory: a lane walks its own spectrum row in 64-byte pieces (16 lines per round; every cache line it touches is used in full by
 * back-to-back loads), twice: pass A shapes the lines and accumulates the autocorrelations (a sliding window of eight shaped lines in
 * registers), pass B filters, takes the maximum and forms the log energies.  Standard layout only (N <= 480); the large layout keeps
 * the wave-per-frame kernel. */
#ifndef LC3_BIG
struct __attribute__((aligned(16))) ShlLds {
    double l10[128 * 3];            /* lc3_fastmath.h: the tables of log10 and 2^x (a lane's 100 + 128 evaluations per frame read them from here) */
    double ex2[64];
    unsigned bob[LC3D_MAX_N / 4];   /* band of a line, one byte each */
    int   pc[LC3D_PLAN_HEAD_WORDS];
};

/* R/tns_coder.c:91-155,279-287 for one filter (rare: total_bits < 480 only).  a[]: Levinson's predictor as tns_levinson leaves it, rc[]: its
 * reflection coefficients; out[0 .. maxOrder) the reflection coefficients of the weighted polynomial.  Index-heavy: private arrays. */
__device__ __attribute__((noinline)) void shl_lpc_weight(const float* a_in, const float* rc_in, float* outp, int maxOrder, float maxPG, float predGain)
{
    float sc[36], pa[9];
    pa[0] = 1;
    for (int j = 1; j <= maxOrder - 1; j++) pa[j] = -a_in[maxOrder - j];
    pa[maxOrder] = rc_in[maxOrder - 1];
    const float alpha = (float)((double)((maxPG - predGain)) * (0.85f - 1.0) / (double)(maxPG - 1.5f) + 1.0);
    for (int i = 0; i <= maxOrder; i++) sc[i] = pa[i] * m_powf(alpha, (float)i);
    int len = maxOrder + 1; const int len0 = len;
    float* pa_ = sc; float* out = sc + 9; float* t0 = sc + 18; float* bf = sc + 26;
    for (int i = 0; i < len - 1; i++) out[i] = 0;
    { float a0 = pa_[0]; for (int i = 0; i < len; i++) { pa_[i] = pa_[i] / a0; a0 = pa_[0]; } }
    out[len - 1] = pa_[len - 1];
    for (int k = len0 - 2; k >= 0; k--) {
        for (int i = 0; i < len - 1; i++) t0[i] = pa_[1 + i];
        int l = len - 1;
        const float knxt = t0[l - 1];
        l = l - 1;
        bf[0] = 1;
        for (int i = 0; i < l; i++) {
            const float t2 = knxt * t0[l - 1 - i];
            bf[i + 1] = (float)((double)(t0[i] - t2) / (1.0 - (double)(fabsf(knxt) * fabsf(knxt))));
        }
        len = l + 1;
        out[k] = bf[len - 1];
        for (int i = 0; i < len; i++) pa_[i] = bf[i];
    }
    for (int i = 0; i < len0 - 1; i++) out[i] = out[i + 1];
    for (int i = 0; i < 8; i++) outp[i] = i < maxOrder ? out[i] : 0.0f;
}

#ifndef SHL_WAVES
#define SHL_WAVES 2
#endif
#ifdef SHL_VGPRS
#define SHL_ATTR __attribute__((amdgpu_waves_per_eu(SHL_WAVES, SHL_WAVES), amdgpu_num_vgpr(SHL_VGPRS)))
#else
#define SHL_ATTR __attribute__((amdgpu_waves_per_eu(SHL_WAVES, SHL_WAVES)))
#endif
#ifdef LC3_ENC_VBW
#define SHL_KERNEL_NAME ERP_FN(lc3_enc_shape_lane_kernel_vbw)   /* per-frame bandwidths (lc3_kernels.hip, -DLC3_ENC_VBW): only this kernel of the file */
#else
#define SHL_KERNEL_NAME ERP_FN(lc3_enc_shape_lane_kernel)
#endif
extern "C" __global__ void __launch_bounds__(WAVE) SHL_ATTR
SHL_KERNEL_NAME(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int RT /* rows per channel-stream */, int r0 /* first row of this launch */, int nt, int ncs,
                          float* __restrict__ rows /* [cs][RT][srow] */, int srow, float* __restrict__ frec /* [cs][RT][FR_WORDS] */
#ifdef LC3_ENC_VBW
                          , const uint16_t* __restrict__ bwf /* [stream][RT] bandwidth in force for each stream-frame, Hz */
#endif
                          LC3_ERP_OPT)
{
    __shared__ ShlLds L;
    const int lane = threadIdx.x;
    ERP_LANE_FRAME(r0, nt)
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    for (int i = lane; i < LC3D_MAX_N; i += WAVE) ((uint8_t*)L.bob)[i] = P->band_of_bin[i];
    for (int i = lane; i < 128 * 3; i += WAVE) L.l10[i] = lc3m_log10_tab[i];
    L.ex2[lane] = lc3m_exp2_tab[lane];
    LSYNC();
#if !defined(LC3_OCML_MATH) && !defined(SHL_GLOBAL_TABLES)
#define m_log10f(x_) lc3m_log10f((x_), L.l10)
#define m_pow2f(x_) lc3m_exp2f((x_), L.ex2)
#endif
#ifndef LC3_ENC_RPIPE
    const long long cf = (long long)blockIdx.x * WAVE + lane;
    const bool valid = cf < (long long)ncs * nt;
    const int cs = valid ? (int)(cf / nt) : 0, t = valid ? r0 + (int)(cf % nt) : r0;
#endif
    float* xr = LC3D_ROW_BASE(rows, cs, t, RT, srow);
#define XP(k_) (&xr[LC3D_ROW_OFF((k_), RT)])
    float* rec = frec + ((size_t)cs * RT + t) * FR_WORDS;
    const lc3d_chan* __restrict__ C = &chans[cs];
    const int ylen = PI(ylen), N = PI(N), nb = PI(nbands), dms = PI(dms), hr = PI(hrmode);
    const int total_bits = C->total_bits, off = C->gg_off;
    /* ---- SNS interpolation R/sns_interpolate_scf.c:13-89: 16 quantised scale factors -> 64 gains -> band gains 2^-g.  A band's gain is formed when the
     *      walk over the lines enters the band (bands are runs of consecutive lines; the band index is wave-uniform) ---- */
    float g[16];
#pragma unroll
    for (int i = 0; i < 16; i += 4) { const float4 v = *(const float4*)&rec[FR_SCFQ + i]; g[i] = v.x; g[i + 1] = v.y; g[i + 2] = v.z; g[i + 3] = v.w; }
    const int dnb = 64 - nb;
    int n4 = 0;
    if (dnb >= 32) { const float ratio = fabsf((float)(1.0 - 32.0 / (double)(float)nb)); n4 = (int)round((double)(ratio * (float)nb)); }
    /* one of the 64 interpolated values; i is wave-uniform */
    auto v64 = [&](int i) -> float {
        float ga, gb; int r;
        if (i < 2) return g[0];
        if (i < 62) { const int n = (i - 2) >> 2; r = (i - 2) & 3; ga = g[n]; gb = g[n + 1]; }
        else { ga = g[15]; gb = g[15]; r = i - 62; const double dd = (double)(g[15] - g[14]); return r == 0 ? (float)((double)ga + dd / 8.0) : (float)((double)ga + 3.0 * dd / 8.0); }
        const double dd = (double)(gb - ga);
        if (r == 0) return (float)((double)ga + dd / 8.0);
        if (r == 1) return (float)((double)ga + 3.0 * dd / 8.0);
        if (r == 2) return (float)((double)ga + 5.0 * dd / 8.0);
        return (float)((double)ga + 7.0 * dd / 8.0);
    };
    auto band_gain = [&](int b) -> float {
        float v;
        if (dnb == 0) v = v64(b);
        else if (dnb < 32) { if (b < dnb) v = (float)((double)(v64(2 * b) + v64(2 * b + 1)) / 2.0); else v = v64(b + dnb); }
        else {
            if (b < n4) v = (float)((double)(v64(4 * b) + v64(4 * b + 1) + v64(4 * b + 2) + v64(4 * b + 3)) / 4.0);
            else { const int i = b - n4; v = (float)((double)(v64(4 * n4 + 2 * i) + v64(4 * n4 + 2 * i + 1)) / 2.0); }
        }
        return m_pow2f(-v);
    };
    /* ---- bandwidth controller R/cutoff_bandwidth.c:13-26 and the TNS geometry R/tns_coder.c:196-246 ---- */
    int bw = ((const int*)rec)[FR_BW];
#ifdef LC3_ENC_VBW
    const int fbw = bwf[(size_t)(cs / PI(channels)) * RT + t];          /* this lane's frame: cut and cbin are per lane here */
    const bool cut = fbw != 0; const int cbin = lc3d_bw_cut_bin(fbw, dms);
    if (cut) bw = imin(bw, lc3d_bw_index(fbw));
#else
    const bool cut = C->bandwidth != 0; const int cbin = C->bw_cut_bin;
    if (cut) bw = imin(bw, C->bw_index);
#endif
    const int bw_bin = lc3t_bw_bins[PI(bw_cls) * 6 + bw];
    int numfilters, start0, start1 = 0, stop0, stop1 = 0, obits_off = 8; float maxPG = 2;
    const int maxOrder = dms == 100 ? 8 : 4, nSub = dms == 100 ? 3 : 2;
    {
        int fs = PI(fs), Nn = N;
        numfilters = (fs >= 32000 && dms >= 50) ? 2 : 1;
        if ((double)Nn > 40 * ((double)(float)dms / 10.0)) { Nn = (int)(40 * ((double)(float)dms / 10.0)); fs = 40000; }
        start0 = (600 * Nn * 2 / fs) + 1;
        if ((dms >= 50 && (double)total_bits >= 48 * ((double)(float)dms / 10.0)) || dms == 25) { maxPG = 1.5f; obits_off = 0; }
        if (bw >= 3 && numfilters == 2) { start1 = bw_bin / 2 + 1; stop0 = bw_bin / 2; stop1 = bw_bin; }
        else { numfilters = 1; stop0 = bw_bin; }
    }
    /* ---- pass A: shape the lines (R/mdct_shaping.c), autocorrelations of the sub-divisions in line order (R/tns_coder.c:18-39,258-277) ---- */
    float R0[9], R1[9];                              /* lag-windowed r[] of the two filters */
#pragma unroll
    for (int k = 0; k < 9; k++) { R0[k] = 0; R1[k] = 0; }
    {
        float acc[9], rr[9], yp[8];
#pragma unroll
        for (int k = 0; k < 9; k++) { acc[k] = 0; rr[k] = 0; }
#pragma unroll
        for (int k = 0; k < 8; k++) yp[k] = 0;
        int cur_b = -1; float cur_g = 1.0f;
        int sf = 0, ssub = 0; bool dead = false;     /* the sub-division being summed: filter, index; `dead`: a zero-energy sub-division ended this filter's sums */
        int slo, shi;
#define SHL_BOUNDS() do { const int fstart_ = sf ? start1 : start0, fstop_ = sf ? stop1 : stop0; \
            const float sublen_ = (float)(((double)(float)fstop_ + 1.0 - (double)(float)fstart_) / (double)(float)nSub); \
            slo = (int)(floor((double)(sublen_ * (float)ssub)) + fstart_ - 1); shi = (int)(floor((double)(sublen_ * (float)(ssub + 1))) + fstart_ - 1); \
            if (sf >= numfilters) { slo = 0x7fffffff; shi = 0x7fffffff; } } while (0)
        SHL_BOUNDS();
        float4 xn[4];
#pragma unroll
        for (int j = 0; j < 4; j++) xn[j] = *(const float4*)XP(4 * j);
        for (int k0 = 0; k0 < ylen; k0 += 16) {
            float xs[16], ys[16];
#pragma unroll
            for (int j = 0; j < 4; j++) { xs[4 * j] = xn[j].x; xs[4 * j + 1] = xn[j].y; xs[4 * j + 2] = xn[j].z; xs[4 * j + 3] = xn[j].w; }
            if (k0 + 16 < ylen) {
#pragma unroll
                for (int j = 0; j < 4; j++) xn[j] = *(const float4*)XP(k0 + 16 + 4 * j);
            }
            const unsigned bw4[4] = {L.bob[(k0 >> 2)], L.bob[(k0 >> 2) + 1], L.bob[(k0 >> 2) + 2], L.bob[(k0 >> 2) + 3]};     /* the bands of these 16 lines (wave-uniform) */
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int b = uni((int)((bw4[j >> 2] >> (8 * (j & 3))) & 255u)), k = k0 + j;
                if (b != cur_b) { cur_b = b; cur_g = b < nb ? band_gain(b) : 1.0f; }
                float y = k < ylen ? xs[j] : 0.0f;
                if (b < nb) y = y * cur_g;
                ys[j] = y;
            }
            if (__any(cut && ylen > cbin && k0 + 16 > cbin - 1)) {          /* bandwidth controller: rare, and only from the cut-off line on */
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const int k = k0 + j;
                    if (cut && ylen > cbin) {
                        if (k >= cbin - 1 && k < cbin + 3) ys[j] = ys[j] * (k == cbin - 1 ? 0.5f : k == cbin ? 0.25f : k == cbin + 1 ? 0.125f : 0.0625f);
                        else if (k >= cbin + 3) ys[j] = 0;
                    }
                }
            }
            /* The shaped lines go back to the row and pass B reads them.  The alternative (-DSHL_RESHAPE_B, tools/variants.sh): no write here, pass B shapes the raw
             * lines again - one multiplication per line, the band gains formed once more.  It takes 0.42 GB per c1 call off the row traffic (6.1 -> 5.7 GB) and is
             * byte-identical, but it is not faster - measured on one box, Mframes/s with / without the write: c1 108.2 / 107.7, c3 87.9 / 85.8, c4 114.5 / 113.7: the
             * call is bound by instructions, not by these bytes (DESIGN.md section 5). */
#ifndef SHL_RESHAPE_B
            if (valid) {
#pragma unroll
                for (int j = 0; j < 4; j++) if (k0 + 4 * j < ylen) *(float4*)XP(k0 + 4 * j) = make_float4(ys[4 * j], ys[4 * j + 1], ys[4 * j + 2], ys[4 * j + 3]);
            }
#endif
            /* autocorrelation terms of these lines.  Fast path: every lane is at least 8 lines into its sub-division for the whole round */
            if (__all(k0 - slo >= 8 && k0 + 16 <= shi)) {
#pragma unroll
                for (int j = 0; j < 16; j++) {
#pragma unroll
                    for (int k = 0; k < 9; k++) { const float h = j - k >= 0 ? ys[j - k >= 0 ? j - k : 0] : yp[8 + j - k >= 0 ? 8 + j - k : 0]; acc[k] += ys[j] * h; }
                }
            } else if (__any(k0 + 16 > slo && k0 <= shi)) {
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const int i = k0 + j;
                    if (__any(i == shi)) {
                        if (i == shi) {                       /* a sub-division ends: its normalised sums go into r[] (R/tns_coder.c:262-277) */
                            if (!dead) {
                                const float e = acc[0];
                                if (e == 0) {
#pragma unroll
                                    for (int k = 0; k < 9; k++) rr[k] = k == 0 ? 1.0f : 0.0f;
                                    dead = true;
                                } else {
#pragma unroll
                                    for (int k = 0; k < 9; k++) rr[k] = rr[k] + acc[k] / e;
                                }
                            }
#pragma unroll
                            for (int k = 0; k < 9; k++) acc[k] = 0;
                            ssub++;
                            if (ssub == nSub) {
#pragma unroll
                                for (int k = 0; k < 9; k++) { const float v = k <= maxOrder ? rr[k] * lc3t_tns_lagwin[k] : 0.0f; if (sf == 0) R0[k] = v; else R1[k] = v; rr[k] = 0; }
                                ssub = 0; sf++; dead = false;
                            }
                            SHL_BOUNDS();
                        }
                    }
                    const int li = i - slo;
                    if (i >= slo && i < shi) {
#pragma unroll
                        for (int k = 0; k < 9; k++) { const float h = j - k >= 0 ? ys[j - k >= 0 ? j - k : 0] : yp[8 + j - k >= 0 ? 8 + j - k : 0]; if (li >= k) acc[k] += ys[j] * h; }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++) yp[k] = ys[8 + k];
        }
        /* a sub-division that ends with the spectrum (shi == ylen) */
        for (int g = 0; g < 6; g++) {
            if (!__any(shi <= ylen && shi != 0x7fffffff)) break;
            if (shi <= ylen && shi != 0x7fffffff) {
                if (!dead) {
                    const float e = acc[0];
                    if (e == 0) {
#pragma unroll
                        for (int k = 0; k < 9; k++) rr[k] = k == 0 ? 1.0f : 0.0f;
                        dead = true;
                    } else {
#pragma unroll
                        for (int k = 0; k < 9; k++) rr[k] = rr[k] + acc[k] / e;
                    }
                }
#pragma unroll
                for (int k = 0; k < 9; k++) acc[k] = 0;
                ssub++;
                if (ssub == nSub) {
#pragma unroll
                    for (int k = 0; k < 9; k++) { const float v = k <= maxOrder ? rr[k] * lc3t_tns_lagwin[k] : 0.0f; if (sf == 0) R0[k] = v; else R1[k] = v; rr[k] = 0; }
                    ssub = 0; sf++; dead = false;
                }
                SHL_BOUNDS();
            }
        }
#undef SHL_BOUNDS
    }
    /* ---- Levinson-Durbin, prediction gain, LPC weighting, coefficient quantisation (R/tns_coder.c:41-168,279-337), per filter ---- */
    float rcq[2][8]; int tidx[2][8]; int ord[2] = {0, 0}; int tns_bits = 0;
#pragma unroll
    for (int f = 0; f < 2; f++) {
#pragma unroll
        for (int i = 0; i < 8; i++) { rcq[f][i] = 0; tidx[f][i] = 0; }
        if (__any(f < numfilters)) {
            float r[9], a[9], rc[8], buf[9];
#pragma unroll
            for (int i = 0; i < 9; i++) { r[i] = f ? R1[i] : R0[i]; a[i] = 0; }
            float g = r[1] / r[0];
            a[0] = g;
            float v = (float)((1.0 - (double)(g * g)) * (double)r[0]);
            rc[0] = -g;
#pragma unroll
            for (int tt = 1; tt < 8; tt++) {
                if (tt < maxOrder) {
                    float sum = 0;
#pragma unroll
                    for (int i = 1; i <= tt; i++) sum += a[i - 1] * r[i];
                    g = (r[tt + 1] - sum) / v;
#pragma unroll
                    for (int j = 1; j <= tt; j++) buf[j] = a[j - 1] - g * a[tt - j];
#pragma unroll
                    for (int j = 1; j <= tt; j++) a[j] = buf[j];
                    a[0] = g;
                    v = v * (1 - g * g);
                    rc[tt] = -g;
                } else rc[tt] = 0;
            }
            const float predGain = r[0] / v;
            const bool live = f < numfilters;
            int tns = live && predGain > 1.5f;
            const bool weight = tns && predGain < maxPG;
            if (__any(weight)) {
                if (weight) { float wout[8]; shl_lpc_weight(a, rc, wout, maxOrder, maxPG, predGain);
#pragma unroll
                    for (int i = 0; i < 8; i++) rc[i] = wout[i]; }
            }
            int idx[8]; float qv[8]; int o = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const float c = i < maxOrder ? rc[i] : 0.0f;
                int ix = 0;
#pragma unroll
                for (int q = 0; q < 17; q++) ix = (c <= lc3t_tns_rc_thr[q + 1] && c > lc3t_tns_rc_thr[q]) ? q : ix;
                if (i >= maxOrder) ix = 0;
                idx[i] = ix;
                qv[i] = (tns && i < maxOrder) ? lc3t_tns_rc_pts[ix] : 0.0f;
                if (qv[i] != 0) o = i + 1;
            }
            if (o == 0) tns = 0;                      /* would be undefined behaviour in the reference (R/tns_coder.c:311-321); filter off */
            int bits = live ? 1 : 0;
            if (tns) {
                int tsum = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) if (i < o) tsum += lc3t_tns_coef_bits[i * 17 + idx[i]];
                bits += (tsum + lc3t_tns_order_bits[obits_off + o - 1] + 2047) >> 11;
            }
            tns_bits += bits;
            ord[f] = tns ? o : 0;
#pragma unroll
            for (int i = 0; i < 8; i++) { rcq[f][i] = live ? qv[i] : 0.0f; tidx[f][i] = (tns && i < o) ? idx[i] : 0; }
        }
    }
    /* ---- pass B: the MA lattice in place (R/tns_coder.c:339-357; its state runs on from filter 0 into filter 1), spectrum maximum, 4-bin log
     *      energies (R/estimate_global_gain.c:52-91; with the high-resolution regulariser a third pass, it needs the sums over all lines) ---- */
    const bool anyf = ord[0] > 0 || ord[1] > 0;
    const bool regul = hr && C->reg_bits > 0;
    float x_max = 0; float M0 = 1e-5f, M1 = 1e-5f;
    {
        /* The lattice without per-line selects: a tap beyond the order in force has coefficient 0 (it leaves the line as it is; its state word
         * keeps what the other filter left there: one select with a mask that changes with the filter only), lines in front of the first filter
         * are skipped (the same line for every frame of a configuration), and where a lane's filter range ends the coefficients become 0 for
         * the rest of its row.  Events - filter 0 hands over to filter 1, the last range ends - are rare: one compare per line. */
        float st[8], rca[8]; bool tm[8];
#pragma unroll
        for (int j = 0; j < 8; j++) { st[j] = 0; rca[j] = rcq[0][j]; tm[j] = j < ord[0]; }
        int phase = 0, nextev = numfilters == 2 ? start1 - 1 : stop0;
        int cur_b = -1; float cur_g = 1.0f;
        float4 xn[4];
#pragma unroll
        for (int j = 0; j < 4; j++) xn[j] = *(const float4*)XP(4 * j);
        for (int k0 = 0; k0 < ylen; k0 += 16) {
            float ys[16];
#pragma unroll
            for (int j = 0; j < 4; j++) { ys[4 * j] = xn[j].x; ys[4 * j + 1] = xn[j].y; ys[4 * j + 2] = xn[j].z; ys[4 * j + 3] = xn[j].w; }
            if (k0 + 16 < ylen) {
#pragma unroll
                for (int j = 0; j < 4; j++) xn[j] = *(const float4*)XP(k0 + 16 + 4 * j);
            }
#ifdef SHL_RESHAPE_B
            {   /* the row still holds the MDCT lines: shape them as pass A did (same operations, same results) */
                const unsigned bw4[4] = {L.bob[(k0 >> 2)], L.bob[(k0 >> 2) + 1], L.bob[(k0 >> 2) + 2], L.bob[(k0 >> 2) + 3]};
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const int b = uni((int)((bw4[j >> 2] >> (8 * (j & 3))) & 255u)), k = k0 + j;
                    if (b != cur_b) { cur_b = b; cur_g = b < nb ? band_gain(b) : 1.0f; }
                    float y = k < ylen ? ys[j] : 0.0f;
                    if (b < nb) y = y * cur_g;
                    ys[j] = y;
                }
                if (__any(cut && ylen > cbin && k0 + 16 > cbin - 1)) {
#pragma unroll
                    for (int j = 0; j < 16; j++) {
                        const int k = k0 + j;
                        if (cut && ylen > cbin) {
                            if (k >= cbin - 1 && k < cbin + 3) ys[j] = ys[j] * (k == cbin - 1 ? 0.5f : k == cbin ? 0.25f : k == cbin + 1 ? 0.125f : 0.0625f);
                            else if (k >= cbin + 3) ys[j] = 0;
                        }
                    }
                }
            }
#endif
#ifdef SHL_RESHAPE_B
            const bool changed = true;
#else
            const bool changed = __any(anyf && k0 + 16 > start0 - 1 && k0 < (numfilters == 2 ? stop1 : stop0));      /* only the rounds the lattice touches go back */
#endif
            if (__any(anyf && k0 + 16 > start0 - 1 && k0 < (numfilters == 2 ? stop1 : stop0))) {
                /* Every tap up to the lane's order runs as a full lattice stage (the reference's last stage only adds: the value it would pass on is
                 * never used); which taps are live is a per-lane mask that changes with the filter, not with the line */
                const int comax = uni(wave_max_i(imax(ord[0], ord[1])));
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const int i = k0 + j;
                    if (i >= start0 - 1) {
                        if (__any(i == nextev)) {
                            if (i == nextev) {
                                if (phase == 0 && numfilters == 2) {
#pragma unroll
                                    for (int q = 0; q < 8; q++) { rca[q] = rcq[1][q]; tm[q] = q < ord[1]; }
                                    nextev = stop1; phase = 1;
                                } else {
#pragma unroll
                                    for (int q = 0; q < 8; q++) { rca[q] = 0; tm[q] = false; }
                                    nextev = 0x7fffffff;
                                }
                            }
                        }
                        float s = ys[j], save = s;
                        if (comax == 8) {            /* the common case at 10 ms: every tap in force somewhere in the wave - no test per tap */
#pragma unroll
                            for (int q = 0; q < 8; q++) {
                                const float tt = rca[q] * s + st[q];
                                s = s + rca[q] * st[q];
                                st[q] = tm[q] ? save : st[q]; save = tt;
                            }
                        } else {
#pragma unroll
                            for (int q = 0; q < 8; q++) {
                                if (q < comax) {
                                    const float tt = rca[q] * s + st[q];
                                    s = s + rca[q] * st[q];
                                    st[q] = tm[q] ? save : st[q]; save = tt;
                                }
                            }
                        }
                        ys[j] = s;
                    }
                }
            }
            if (valid && changed) {
#pragma unroll
                for (int j = 0; j < 4; j++) if (k0 + 4 * j < ylen) *(float4*)XP(k0 + 4 * j) = make_float4(ys[4 * j], ys[4 * j + 1], ys[4 * j + 2], ys[4 * j + 3]);      /* behind line ylen the row holds the log energies */
            }
            float e4[4];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const float y = k0 + j < ylen ? ys[j] : 0.0f;
                x_max = fmaxf(x_max, fabsf(y));
                if (regul && k0 + j < ylen) { const double ax = fabs((double)y); M0 = (float)((double)M0 + ax); M1 = (float)((double)M1 + (double)(k0 + j) * ax); }
            }
            if (!regul) {
#if !defined(LC3_OCML_MATH) && !defined(SHL_GLOBAL_TABLES)
                /* four logarithms without a branch between them (their table reads overlap); an argument that is not a positive finite number - a NaN in the
                 * spectrum - takes the general function behind the group */
                float ta[4], lg[4]; int sp = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float tt = ys[4 * q] * ys[4 * q];
                    tt += ys[4 * q + 1] * ys[4 * q + 1]; tt += ys[4 * q + 2] * ys[4 * q + 2]; tt += ys[4 * q + 3] * ys[4 * q + 3];
                    ta[q] = tt + 0.0f + PF(c_2m31);
                }
#pragma unroll
                for (int q = 0; q < 4; q++) { int s1; lg[q] = lc3m_log10f_nb(ta[q], L.l10, &s1); sp |= s1; }
                if (__any(sp != 0)) {
#pragma unroll
                    for (int q = 0; q < 4; q++) lg[q] = m_log10f(ta[q]);
                }
#pragma unroll
                for (int q = 0; q < 4; q++) e4[q] = (float)((28.0 / 20.0) * (7 + 10.0 * (double)lg[q]));
#else
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float tt = ys[4 * q] * ys[4 * q];
                    tt += ys[4 * q + 1] * ys[4 * q + 1]; tt += ys[4 * q + 2] * ys[4 * q + 2]; tt += ys[4 * q + 3] * ys[4 * q + 3];
                    e4[q] = (float)((28.0 / 20.0) * (7 + 10.0 * (double)m_log10f(tt + 0.0f + PF(c_2m31))));
                }
#endif
                if (valid) *(float4*)XP(ylen + (k0 >> 2)) = make_float4(e4[0], e4[1], e4[2], e4[3]);
            }
        }
    }
    if (__any(regul)) {
        const float thresh = 2 * PF(frame_ms);
        const float q = M1 / M0;
        const float rB = 8 * (1 - (q < thresh ? q : thresh) / thresh);
        const float reg_val = regul ? x_max * m_powf(2.0f, (float)(-C->reg_bits) - rB) : 0.0f;
        for (int k0 = 0; k0 < ylen; k0 += 16) {
            float ys[16], e4[4];
#pragma unroll
            for (int j = 0; j < 4; j++) { const float4 v = *(const float4*)XP(k0 + 4 * j); ys[4 * j] = v.x; ys[4 * j + 1] = v.y; ys[4 * j + 2] = v.z; ys[4 * j + 3] = v.w; }
#pragma unroll
            for (int q2 = 0; q2 < 4; q2++) {
                float tt = ys[4 * q2] * ys[4 * q2];
                tt += ys[4 * q2 + 1] * ys[4 * q2 + 1]; tt += ys[4 * q2 + 2] * ys[4 * q2 + 2]; tt += ys[4 * q2 + 3] * ys[4 * q2 + 3];
                e4[q2] = (float)((28.0 / 20.0) * (7 + 10.0 * (double)m_log10f(tt + reg_val + PF(c_2m31))));
            }
            if (valid && regul) *(float4*)XP(ylen + (k0 >> 2)) = make_float4(e4[0], e4[1], e4[2], e4[3]);
        }
    }
    float ind_min = (float)off;
    if (x_max != 0) {
        const float g_min = hr == 1 ? x_max / (float)(32768 * 256 - 2) : (float)((double)x_max / (32768 - 0.375));
        ind_min = (float)ceil(28.0 * (double)m_log10f(g_min));
    }
    if (valid) {
        int* ri = (int*)rec;
        *(int4*)&ri[FR_TNS] = make_int4(numfilters, ord[0], ord[1], tns_bits);
#pragma unroll
        for (int f = 0; f < 2; f++) {
            *(int4*)&ri[FR_TNS + 4 + 8 * f] = make_int4(tidx[f][0], tidx[f][1], tidx[f][2], tidx[f][3]);
            *(int4*)&ri[FR_TNS + 8 + 8 * f] = make_int4(tidx[f][4], tidx[f][5], tidx[f][6], tidx[f][7]);
        }
        ri[FR_GGMIN] = __float_as_int(ind_min); ri[FR_XZERO] = x_max == 0 ? 1 : 0; ri[FR_BWC] = bw;
    }
#undef XP
#undef m_log10f
#undef m_pow2f
}
#endif

#if !defined(LC3_BIG) && !defined(LC3_ENC_VBW)
/* lc3_enc_scf_lane_kernel -- per-band energies (R/per_band_energy.c:13-30), bandwidth detector (R/detect_cutoff_warped.c:13-83) and SNS scale
 * factors (R/sns_compute_scf.c:13-176), one channel-frame per LANE.  In the wave-per-frame front these stages are short serial walks over 64
 * (or fewer) values - 64-term ordered sums read lane by lane, the detector's band walk, the 6-tap down-sampling - about 720 instructions per
 * frame on the vector and scalar units; per lane they are the reference's loops, 64 frames to an instruction.  A frame's 64 band energies live
 * in LDS ([band][lane]: conflict-free).  in: the MDCT spectrum row; out: FR_SCF[16], FR_BW of the frame's record. */
struct __attribute__((aligned(16))) ScfLds {
    float en[64 * 64];
    int   be[68];               /* band edges */
    int   pc[LC3D_PLAN_HEAD_WORDS];
};
#ifndef SCF_WAVES
#define SCF_WAVES 3
#endif
extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(SCF_WAVES, SCF_WAVES)))
ERP_FN(lc3_enc_scf_lane_kernel)(const lc3d_plan* __restrict__ P, int RT, int r0, int nt, int ncs, const float* __restrict__ rows /* [cs][RT][srow] */, int srow, float* __restrict__ frec,
                        int with_vq /* the SNS quantiser of the frame behind its scale factors (no stream of the batch has attack handling: nothing sits between the two) */ LC3_ERP_OPT)
{
    __shared__ ScfLds L;
    const int lane = threadIdx.x;
    ERP_LANE_FRAME(r0, nt)
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    LSYNC();
    const int nb0 = PI(nbands), ylen = PI(ylen);
    for (int i = lane; i < 68; i += WAVE) L.be[i] = i <= nb0 ? (int)lc3t_band_pool[PI(band_off) + i] : 0x7fffffff;
    LSYNC();
#ifndef LC3_ENC_RPIPE
    const long long cf = (long long)blockIdx.x * WAVE + lane;
    const bool valid = cf < (long long)ncs * nt;
    const int cs = valid ? (int)(cf / nt) : 0, t = valid ? r0 + (int)(cf % nt) : r0;
#endif
    const float* xr = LC3D_ROW_BASE(rows, cs, t, RT, srow);
#define XP(k_) (&xr[LC3D_ROW_OFF((k_), RT)])
    float* rec = frec + ((size_t)cs * RT + t) * FR_WORDS;
    /* ---- band energies: the lines in order, a band closes where the next one starts (wave-uniform) ---- */
    {
        int b = 0, edge = uni(L.be[1]), lo = uni(L.be[0]);
        float sum = 0;
        float4 xn[4];
#pragma unroll
        for (int j = 0; j < 4; j++) xn[j] = *(const float4*)XP(4 * j);
        for (int k0 = 0; k0 < ylen; k0 += 16) {
            float xs[16];
#pragma unroll
            for (int j = 0; j < 4; j++) { xs[4 * j] = xn[j].x; xs[4 * j + 1] = xn[j].y; xs[4 * j + 2] = xn[j].z; xs[4 * j + 3] = xn[j].w; }
            if (k0 + 16 < ylen) {
#pragma unroll
                for (int j = 0; j < 4; j++) xn[j] = *(const float4*)XP(k0 + 16 + 4 * j);
            }
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int k = k0 + j;
                while (k == edge) {            /* wave-uniform; `while`: a band may be empty */
                    L.en[b * 64 + lane] = sum / (float)(edge - lo);
                    sum = 0; b++; lo = edge; edge = uni(L.be[b + 1]);
                }
                if (k < ylen) sum += xs[j] * xs[j];
            }
        }
        while (b < nb0) { L.en[b * 64 + lane] = sum / (float)(edge - lo); sum = 0; b++; lo = edge; edge = uni(L.be[b + 1]); }
    }
    /* ---- bandwidth detector ---- */
    int bw = PI(fs_idx);
    if (PI(fs_idx) > 0 && PI(hrmode) == 0) {
        const int f = PI(fs_idx);
        const uint8_t* st = &lc3t_bw_start[(PI(bw_cls) * 4 + f - 1) * 4]; const uint8_t* sp = &lc3t_bw_stop[(PI(bw_cls) * 4 + f - 1) * 4];
        int counter = f;
        float sum = 0;
        for (int i = st[counter - 1]; i <= sp[counter - 1]; i++) sum += L.en[i * 64 + lane];
        float mean = sum / (float)(sp[counter - 1] - st[counter - 1] + 1);
        while (mean < (float)lc3t_bw_quiet_thr[counter - 1]) {
            counter--;
            if (counter == 0) break;
            sum = 0;
            for (int i = st[counter - 1]; i <= sp[counter - 1]; i++) sum += L.en[i * 64 + lane];
            mean = sum / (float)(sp[counter - 1] - st[counter - 1] + 1);
        }
        bw = counter;
        if (bw < f) {
            const float thr = (float)lc3t_bw_brick_thr[counter];
            const int stop = st[counter], dist = lc3t_bw_brick_dist[counter];
            int brick = 0;
            for (int i = stop; i >= stop - dist; i--) {
                const float ediff = (float)(10.0 * (double)m_log10f(L.en[(i - dist + 1) * 64 + lane] + 1.1920928955078125e-07f) -
                                            10.0 * (double)m_log10f(L.en[(i + 1) * 64 + lane] + 1.1920928955078125e-07f));
                if (ediff > thr) { brick = 1; break; }
            }
            if (!brick) bw = f;
        }
    }
    /* ---- scale factors.  c(i): the energies spread over 64 bands (R/sns_compute_scf.c:30-60) ---- */
    const int d = 64 - nb0;
    int n4 = 0;
    if (d > 0 && d >= nb0) { const float ratio = fabsf((float)(1.0 - 32.0 / (double)(float)nb0)); n4 = (int)round((double)(ratio * (float)nb0)); }
    auto src = [&](int i) -> int { return d == 0 ? i : d < nb0 ? (i < 2 * d ? i >> 1 : i - d) : (i < 4 * n4 ? i >> 2 : n4 + ((i - 4 * n4) >> 1)); };
    auto sval = [&](int i, float cm, float c, float cp) -> float {
        (void)i;
        return (float)(0.5 * (double)c + 0.25 * (double)cm + 0.25 * (double)cp);
    };
    float ssum = 0;
    {
        float cm = L.en[src(0) * 64 + lane], c = cm, cp = L.en[src(1) * 64 + lane];
        for (int i = 0; i < 64; i++) {
            float s = sval(i, cm, c, cp);
            s = s * P->sns_preemph[i];
            ssum += s;
            cm = c; c = cp; cp = i + 2 < 64 ? L.en[src(i + 2) * 64 + lane] : cp;
        }
    }
    float nf = (ssum / (float)64) * PF(c_1em4);
    nf = nf > PF(c_2m32) ? nf : PF(c_2m32);
    float v4[16];
    {
        const float W[6] = {(float)(1.0 / 12.0), (float)(2.0 / 12.0), (float)(3.0 / 12.0), (float)(3.0 / 12.0), (float)(2.0 / 12.0), (float)(1.0 / 12.0)};
        float cm = L.en[src(0) * 64 + lane], c = cm, cp = L.en[src(1) * 64 + lane];
        float xw[6];                            /* the last six log values: xl[i - 5 .. i] */
#pragma unroll
        for (int q = 0; q < 6; q++) xw[q] = 0;
#pragma unroll
        for (int i = 0; i < 64; i++) {
            float s = sval(i, cm, c, cp);
            s = s * P->sns_preemph[i];
            if (s < nf) s = nf;
            const float xl = (float)((double)m_log2f(s) / 2.0);
            cm = c; c = cp; cp = i + 2 < 64 ? L.en[src(i + 2) * 64 + lane] : cp;
#pragma unroll
            for (int q = 0; q < 5; q++) xw[q] = xw[q + 1];
            xw[5] = xl;
            if (i == 0) xw[4] = xl;              /* band -1 reads band 0 (R/sns_compute_scf.c:122) */
            /* v4[n] = sum_q xl[clamp(4n - 1 + q)] W[q]: complete when xl[4n + 4] has arrived (n < 15), or with the last band repeated (n = 15) */
            if (i >= 4 && (i & 3) == 0) {
                const int n = (i >> 2) - 1;
                float a = 0;
#pragma unroll
                for (int q = 0; q < 6; q++) a += xw[q] * W[q];
                v4[n] = a;
            }
            if (i == 63) {
                float a = 0;
#pragma unroll
                for (int q = 0; q < 5; q++) a += xw[q + 1] * W[q];
                a += xw[5] * W[5];
                v4[15] = a;
            }
        }
        }
    float sum = 0;
#pragma unroll
    for (int n = 0; n < 16; n++) sum += v4[n];
    const float mean = (float)((double)sum / ((double)(float)64 / 4.0));
    float env[16];
#pragma unroll
    for (int n = 0; n < 16; n++) env[n] = PF(sns_damping) * (v4[n] - mean);
    if (valid) {
#pragma unroll
        for (int n = 0; n < 16; n += 4) *(float4*)&rec[FR_SCF + n] = make_float4(env[n], env[n + 1], env[n + 2], env[n + 3]);
        ((int*)rec)[FR_BW] = bw;
    }
    if (with_vq) {               /* wave-uniform */
        if (valid) snsvq_frame(P, env, rec);
    }
#undef XP
}
#endif
