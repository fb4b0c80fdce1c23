/* lc3_enc_snsvq.inc -- SNS vector quantiser, one channel-frame per LANE (included by lc3_kernels.hip).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  process_snsQuantizesScf_Enc (R/sns_quantize_scf.c:165-430) with its
 * pulse searches (pvq_subpyr_search :43-136), MPVQ enumeration (pvq_enc :138-163), DCT-II(16) (R/dct4.c:28-48) and IDCT-II (:19-41).
 * The quantiser turns 16 scale factors into 7 indices and 16 quantised scale factors and depends on nothing else - no encoder
 * state, no spectrum - but almost every step of it is a short serial chain (greedy pulse placement, first-minimum scans, ordered
 * 16-term sums).  Inside lc3_encode_kernel a whole wave walks those chains for one frame (about 1 650 vector instructions, the
 * largest stage of that kernel); here every lane runs the reference's own scalar algorithm for its frame, so one instruction stream
 * serves 64 frames.  Everything a lane needs lives in its registers (arrays are indexed by unrolled loop counters only; the pulse
 * that wins a round is applied with selects), the tables are read at wave-uniform addresses (scalar loads) except the MPVQ offsets.
 *
 * in / out: record `rec` of the frame (FR_* in lc3_plan.h): FR_SCF[16] (+ FR_ATTFLAG) -> FR_SCFQ[16], FR_IDX[7]. */

#ifndef VQ_WAVES
#define VQ_WAVES 4          /* 128 registers: alone the kernel is fastest with 196; beside the other kernels of the pipelined path (runs of 8 frames) 4: 70.2, 5: 69.7, 3: 69.8, 2: 68.5, 6 / 8: 69.3 Mframes/s */
#endif
/* R/sns_quantize_scf.c:43-136 for one search: x[DIM] -> y[DIM] (signed pulses), yn[DIM] (normalised); arrays live in registers */
template <int DIM, int K> __device__ __forceinline__ void vq_pvq(const float* x, float eps, int* y, float* yn)
{
    float xabs[DIM], yf[DIM]; bool neg[DIM];
    float xsum = 0;
#pragma unroll
    for (int i = 0; i < DIM; i++) { xabs[i] = fabsf(x[i]); neg[i] = !(x[i] >= 0); }
#pragma unroll
    for (int i = 0; i < DIM; i++) xsum += xabs[i];
    float yy = 0;
    if (xsum > eps) {
        int tot = 0; float xy = 0;
        const float proj = (float)(K - 1) / xsum;
#pragma unroll
        for (int i = 0; i < DIM; i++) {
            yf[i] = floorf(xabs[i] * proj);                 /* a small integer, exact in float */
            tot += (int)yf[i];
            yy = yy + yf[i] * yf[i];
            xy = xy + xabs[i] * yf[i];
        }
        yy = yy * 0.5f;
        while (tot < K) {
            yy = yy + 0.5f;
            float cnum, cden, bx, by; int best = 0;
            { float a = xy + xabs[0]; a = a * a; cnum = a; cden = yy + yf[0]; bx = xabs[0]; by = yf[0]; }   /* candidate 0 always beats the initial (-2^15, 0) */
#pragma unroll
            for (int i = 1; i < DIM; i++) {
                float a = xy + xabs[i]; a = a * a;
                const float b = yy + yf[i];
                const bool t = a * cden > b * cnum;
                cnum = t ? a : cnum; cden = t ? b : cden; best = t ? i : best; bx = t ? xabs[i] : bx; by = t ? yf[i] : by;
            }
            xy = xy + bx; yy = yy + by; tot++;
#pragma unroll
            for (int i = 0; i < DIM; i++) yf[i] = (i == best) ? yf[i] + 1.0f : yf[i];
        }
        yy = yy * 2.0f;
    } else {
        /* all-zero target: the reference puts the pulses at y[0] and (out of range) y[dim]; only y[0] is ever read back */
        const int y0z = K / 2, ydz = -(K - K / 2);
#pragma unroll
        for (int i = 0; i < DIM; i++) yf[i] = i == 0 ? (float)y0z : 0.0f;
        yy = DIM > 1 ? (float)(y0z * y0z + ydz * ydz) : (float)(K * K);
    }
    const float g = (float)(1.0 / (double)sqrtf(yy));
#pragma unroll
    for (int i = 0; i < DIM; i++) { const int v = neg[i] ? -(int)yf[i] : (int)yf[i]; y[i] = v; yn[i] = (float)v * g; }
}

/* R/sns_quantize_scf.c:19-41 */
__device__ __forceinline__ void vq_idct16(const lc3d_plan* __restrict__ P, float n1, float n2, const float* in, float* out)
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        float sum = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            float t = (float)((double)in[j] * P->idct_cos[i * 16 + j]);
            if (j == 0) t *= n2;
            sum += t;
        }
        out[i] = n1 * sum;
    }
}

/* R/sns_quantize_scf.c:138-163 over pulses[0 .. LEN) */
template <int LEN> __device__ __forceinline__ void vq_mpvq(const int* pulses, int& ls, int& idx)
{
    int k = 0; ls = -1; idx = 0;
#pragma unroll
    for (int pos = LEN - 1; pos >= 0; pos--) {
        const int pv = pulses[pos];
        if (ls >= 0 && pv != 0) idx = 2 * idx + ls;
        if (pv > 0) ls = 0;
        if (pv < 0) ls = 1;
        idx = idx + (int)lc3t_mpvq_offs[(LEN - pos - 1) * 11 + k];
        k += pv < 0 ? -pv : pv;
    }
}

/* the quantiser of one frame: env[16] = the scale factors (smoothed already where the attack detector asked for it) -> FR_SCFQ[16], FR_IDX[7] of the frame's record r.
 * Shared by lc3_enc_snsvq_kernel and, where no stream of the batch has attack handling, by the tail of lc3_enc_scf_lane_kernel (lc3_enc_shapel.inc). */
__device__ __forceinline__ void snsvq_frame(const lc3d_plan* __restrict__ P, const float* env, float* __restrict__ r)
{
    const float eps = __int_as_float(((const int*)P)[offsetof(lc3d_plan, c_2m24) / 4]);
    const float big = __int_as_float(((const int*)P)[offsetof(lc3d_plan, c_2p15) / 4]), sqrt2 = __int_as_float(((const int*)P)[offsetof(lc3d_plan, c_sqrt2) / 4]);
    const float n1 = __int_as_float(((const int*)P)[offsetof(lc3d_plan, c_idct_n1) / 4]), n2 = __int_as_float(((const int*)P)[offsetof(lc3d_plan, c_idct_n2) / 4]);
    int index[7];
    float st1[16], tgtp[16], tgt[16];
    /* ---- stage 1: first minimum over 32 codewords, two halves (R/sns_quantize_scf.c:190-217) ---- */
#pragma unroll
    for (int sec = 0; sec < 2; sec++) {
        const float* cb = sec ? lc3t_sns_hf : lc3t_sns_lf;
        float best = 0; int bi = 0;
        for (int c = 0; c < 32; c++) {
            float sum = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) { const float d = env[8 * sec + i] - cb[c * 8 + i]; sum += d * d; }
            const bool t = c == 0 || sum < best;
            best = t ? sum : best; bi = t ? c : bi;
        }
        index[sec] = bi;
#pragma unroll
        for (int i = 0; i < 8; i++) { const float s = cb[bi * 8 + i]; st1[8 * sec + i] = s; tgtp[8 * sec + i] = env[8 * sec + i] - s; }
    }
    /* ---- DCT-II(16) of the residual, R/dct4.c:28-48 ---- */
    {
        float z[32];
#pragma unroll
        for (int i = 0; i < 8; i++) { z[2 * i] = tgtp[2 * i]; z[2 * i + 1] = 0; z[2 * (15 - i)] = tgtp[2 * i + 1]; z[2 * (15 - i) + 1] = 0; }
        dft16(z);
#pragma unroll
        for (int i = 0; i < 16; i++) tgt[i] = z[2 * i] * P->dct2_tw[2 * i] - z[2 * i + 1] * P->dct2_tw[2 * i + 1];
        tgt[0] = tgt[0] / sqrt2;
    }
    /* ---- the four pulse searches ---- */
    int pA[10], pB[6], pN[16], pF[16];
    float nA[10], nB[6], nN[16], nF[16];
    vq_pvq<10, 10>(tgt, eps, pA, nA);
    vq_pvq<6, 1>(tgt + 10, eps, pB, nB);
    vq_pvq<16, 8>(tgt, eps, pN, nN);
    vq_pvq<16, 6>(tgt, eps, pF, nF);
    /* ---- split shape: gains, error in the DCT domain, IDCT (R/sns_quantize_scf.c:230-330) ---- */
    float yCn[16];
    {
        float sumy = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) { const int yc = i < 10 ? pA[i] : pB[i - 10]; sumy += (float)(yc * yc); }
        const float gf = (float)(1.0 / (double)sqrtf(sumy));
#pragma unroll
        for (int i = 0; i < 16; i++) yCn[i] = (float)(i < 10 ? pA[i] : pB[i - 10]) * gf;
    }
    int idx = 0; float min_err = big;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const float gq = c < 2 ? lc3t_sns_gain_reg[c] : lc3t_sns_gain_reg_lf[c - 2];
        float sum = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) { const float v = gq * (c < 2 ? yCn[j] : (j < 10 ? nA[j] : 0.0f)); const float d = tgt[j] - v; sum += d * d; }
        const bool t = sum < min_err;
        min_err = t ? sum : min_err; idx = t ? c : idx;
    }
    const float glob0 = lc3t_sns_gain_q[idx];
    float cand[16], split[16], subN[16], subF[16];
    {
        const float gq = idx < 2 ? lc3t_sns_gain_reg[idx] : lc3t_sns_gain_reg_lf[idx - 2];
#pragma unroll
        for (int j = 0; j < 16; j++) cand[j] = (gq * (idx < 2 ? yCn[j] : (j < 10 ? nA[j] : 0.0f))) / glob0;
    }
    vq_idct16(P, n1, n2, cand, split);
    vq_idct16(P, n1, n2, nN, subN);
    vq_idct16(P, n1, n2, nF, subF);
    int sub_mode = 0, sub_gain = 0, shape = -1;      /* shape: 0 = yC, 1 = pA only, 2 = near, 3 = far, -1 = none */
    float e_sofar = big, g_sel = 0;
    {
        float s = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) { const float d = tgtp[j] - glob0 * split[j]; s += d * d; }
        if (s < e_sofar) {
            if (idx <= 1) { sub_mode = 0; sub_gain = idx; shape = 0; } else { sub_mode = 1; sub_gain = idx - 2; shape = 1; }
            g_sel = glob0; e_sofar = s;
        }
    }
    {
        float me = big; int gi = idx; float gg = glob0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float g = lc3t_sns_gain_near[i];
            float s = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) s += (tgtp[j] - g * subN[j]) * (tgtp[j] - g * subN[j]);
            const bool t = s < me; me = t ? s : me; gi = t ? i : gi; gg = t ? g : gg;
        }
        if (me < e_sofar) { sub_mode = 2; sub_gain = gi; shape = 2; g_sel = gg; e_sofar = me; }
        me = big;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float g = lc3t_sns_gain_far[i];
            float s = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) s += (tgtp[j] - g * subF[j]) * (tgtp[j] - g * subF[j]);
            const bool t = s < me; me = t ? s : me; gi = t ? i : gi; gg = t ? g : gg;
        }
        if (me < e_sofar) { sub_mode = 3; sub_gain = gi; shape = 3; g_sel = gg; }
    }
    /* ---- quantised scale factors, the selected pulse vector and its enumeration ---- */
    int pulses[16];
    float4 q[4];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const float vs = shape == 0 || shape == 1 ? split[i] : shape == 2 ? subN[i] : subF[i];
        const float st2 = shape >= 0 ? g_sel * vs : 0.0f;
        ((float*)q)[i] = st1[i] + st2;
        pulses[i] = shape == 0 ? (i < 10 ? pA[i] : pB[i - 10]) : shape == 1 ? (i < 10 ? pA[i] : 0) : shape == 2 ? pN[i] : shape == 3 ? pF[i] : 0;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) *(float4*)&r[FR_SCFQ + 4 * i] = q[i];
    int ls10, mi10, ls16, mi16, a6, b6;
    vq_mpvq<10>(pulses, ls10, mi10);
    vq_mpvq<16>(pulses, ls16, mi16);
    vq_mpvq<6>(pulses + 10, a6, b6);
    index[2] = sub_mode; index[3] = sub_gain;
    index[4] = sub_mode < 2 ? ls10 : ls16; index[5] = sub_mode < 2 ? mi10 : mi16;
    index[6] = sub_mode == 0 ? b6 * 2 + a6 : sub_mode == 2 ? -1 : -2;
    int* ri = (int*)&r[FR_IDX];
#pragma unroll
    for (int i = 0; i < 7; i++) ri[i] = index[i];
}

extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(VQ_WAVES, VQ_WAVES)))
ERP_FN(lc3_enc_snsvq_kernel)(const lc3d_plan* __restrict__ P, float* __restrict__ rec /* [cs][RT][FR_WORDS], frame t = row r0 + t */, int RT, int r0, int tb, int nt, int ncs, int with_attack LC3_ERP_OPT)
{
    const long long cf = (long long)blockIdx.x * WAVE + threadIdx.x;          /* frames tb ... tb + nt - 1 of every channel-stream */
    if (cf >= (long long)ncs * nt) return;
#ifdef LC3_ENC_RPIPE                /* ragged: a lane whose frame is absent has nothing to do (every lane is on its own here) */
    if (tb + (int)(cf % nt) >= cnt[(int)(cf / nt) / P->channels]) return;
#endif
    float* r = rec + ((cf / nt) * RT + r0 + tb + cf % nt) * FR_WORDS;
    float env[16];
#pragma unroll
    for (int i = 0; i < 16; i += 4) { const float4 v = *(const float4*)&r[FR_SCF + i]; env[i] = v.x; env[i + 1] = v.y; env[i + 2] = v.z; env[i + 3] = v.w; }
    if (with_attack && ((const int*)r)[FR_ATTFLAG]) {
        /* the attack detector asked for smoothed scale factors (R/sns_compute_scf.c:154-175; the front kernel left the plain ones) */
        const float damp = __int_as_float(((const int*)P)[offsetof(lc3d_plan, att_damping) / 4]);
        float gs[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (i == 0) gs[i] = (float)((double)(env[0] + env[1] + env[2]) / 3.0);
            else if (i == 1) gs[i] = (float)((double)(env[0] + env[1] + env[2] + env[3]) / 4.0);
            else if (i == 14) gs[i] = (float)((double)(env[12] + env[13] + env[14] + env[15]) / 4.0);
            else if (i == 15) gs[i] = (float)((double)(env[13] + env[14] + env[15]) / 3.0);
            else gs[i] = (float)((double)(env[i - 2] + env[i - 1] + env[i] + env[i + 1] + env[i + 2]) / 5.0);
        }
        float sum = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) sum += gs[i];
        const float mean = sum / (float)16;
#pragma unroll
        for (int i = 0; i < 16; i++) env[i] = damp * (gs[i] - mean);
    }
    snsvq_frame(P, env, r);
}
