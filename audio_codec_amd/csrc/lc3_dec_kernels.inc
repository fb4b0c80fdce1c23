/* lc3_dec_kernels.inc -- the stateful and the transform part of the float DECODER on gfx950 (included by lc3_kernels.hip in both
 * kernel layouts; the large layout serves 96 kHz at 5 / 10 ms, which is always high-resolution mode, i.e. without LTPF).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  The decoder (Dec_LC3_Channel_fl, R/dec_lc3_fl.c:13-130) is four kernels,
 * each stage in the mapping that fits its dependences:
 *   lc3_dec_parse_kernel   (lc3_dec_parse.inc) one stream-frame per LANE: everything serial inside a frame but stateless across frames
 *   lc3_dec_plc_kernel     one channel-stream per LANE, frames in order: the concealment bookkeeping (R/plc_main.c, R/plc_update.c),
 *                          which depends on the sequence of bad-frame flags only
 *   lc3_dec_imdct_kernel   one channel-frame per WAVE, all frames of the launch at once: SNS shaping, the concealed spectrum of a
 *                          lost frame (R/plc_noise_substitution0.c), DCT-IV + window (R/imdct.c) without the overlap-add
 *   lc3_dec_synth_kernel   one channel-stream per WAVE, frames in order: overlap-add, LTPF synthesis (R/ltpf_decoder.c), output
 * Records, spectra and windowed frames travel through HBM between them. */

/* -DLC3_DEC_RAGGED (the four _rag objects): per-stream frame counts (lc3plus_dec_batch_set_frame_counts).  The stateful and the transform kernels once more, named
 * with _rag, taking cnt [stream] behind their own parameters - the frames of stream s present in this call, clamped to 0 ... T by the ragged plan kernel: where the
 * dense kernel's frame loop ends at T, theirs ends at cnt[s] (DEC_TC).  Rows and records keep the call's T as their layout. */
#ifdef LC3_DEC_RAGGED
#define DEC_RAG(a) a##_rag
#define DEC_TC(strm_) cnt[strm_]
#else
#define DEC_RAG(a) a
#define DEC_TC(strm_) T
#endif
#ifdef LC3_BIG
#define DEC_IMDCT_KERNEL DEC_RAG(lc3_dec_imdct_kernel_big)
#define DEC_IMDCT_WAVES 3
#define DEC_SYNTH_NAME DEC_RAG(lc3_dec_synth_kernel_big)
#else
#define DEC_IMDCT_KERNEL DEC_RAG(lc3_dec_imdct_kernel)
#define DEC_IMDCT_WAVES 4
#define DEC_SYNTH_NAME DEC_RAG(lc3_dec_synth_kernel)
#endif
/* -DLC3_PCM_PLACED (the two plain _plc objects): the synthesis kernel alone, named with _plc, writing each frame at its offset (lc3_plan.h: lc3d_pcm_placed_*) or,
 * where that is invalid, not at all; nothing else of the frame's decoding differs. */
#ifdef LC3_PCM_PLACED
#define DEC_SYNTH_KERNEL LC3_FMT_CAT(DEC_SYNTH_NAME)
#else
#define DEC_SYNTH_KERNEL DEC_SYNTH_NAME
#endif
#define NR ((MAXN + 63) / 64)                        /* spectrum / time samples per lane */
#define NH ((MAXN / 2 + 63) / 64)                    /* complex DFT points per lane */
#define NM ((MEMCAP + 63) / 64)                      /* overlap-memory samples per lane */
#ifdef LC3_BIG
#define OV_ROW(N) OV_ROW_BIG
#else
#define OV_ROW(N) OV_ROW_STD
#endif

struct __attribute__((aligned(16))) ImdLds {         /* lc3_dec_imdct_kernel: the encoder's member names, so its DFT stages apply */
    static constexpr int XOFF = MEMCAP;
    float xbuf[MEMCAP + MAXN];           /* only the X half is used (XCUR) */
    float A[MAXN];                       /* spectrum -> DFT output -> time-domain aliasing buffer */
    float nrow[MAXN]; float gi[64]; int isc[64];     /* hand-over of the next frame, filled by LDS-DMA while this frame is transformed */
    unsigned char bsel[MAXN];            /* SNS band of a bin, 255 where the bin is not shaped (R/mdct_shaping.c) */
    int pc[LC3D_PLAN_HEAD_WORDS];
};
struct __attribute__((aligned(16))) SynLds {         /* lc3_dec_synth_kernel */
    float lxh[16];                       /* LTPF input history, right-aligned: directly in front of A, which holds the frame after the overlap-add */
    float A[MAXN];
#ifdef LC3_BIG
    float ly[16];                        /* no LTPF in high-resolution mode */
#else
    float ly[DEC_LY + 480];              /* LTPF: [output history | this frame's output] */
#endif
    float sc[160];
    int pc[LC3D_PLAN_HEAD_WORDS]; int st[16]; int isc[64];
#ifdef LC3_STAGE_TIMING
    long long tacc[16];
#endif
};
static_assert(offsetof(SynLds, A) == offsetof(SynLds, lxh) + 64 && offsetof(SynLds, A) % 16 == 0, "LTPF input history must sit directly in front of A");
#ifdef LC3_STAGE_TIMING
#define DTICK(id) do { long long now_ = clock64(); if (lane == 0) L.tacc[id] += now_ - tlast; tlast = now_; } while (0)
#else
#define DTICK(id) do { } while (0)
#endif
#define DPI(f) uni(L.pc[offsetof(lc3d_plan, f) / 4])
#define DPF(f) __int_as_float(uni(L.pc[offsetof(lc3d_plan, f) / 4]))

/* forward complex DFT of N/2 points, X -> A: the encoder's stages (same plan, same LDS member names) */
__device__ __forceinline__ void dec_dft(const lc3d_plan* __restrict__ P, ImdLds& L, int lane)
{
    const int N = DPI(N);
#ifdef LC3_BIG
    if (N == 960) { mdct_dft480_cols(L, lane); mdct_dft480_rows(L, lane); } else
#endif
    if (N == 480) { mdct_dft240_cols(L, lane); mdct_dft240_rows(L, lane); }
    else if (N == 120) mdct_dft60(P, L, lane);
    else { if (N == 320) mdct_dft160_stage1(P, L, lane); else if (N == 160) mdct_dft80_stage1(P, L, lane); mdct_dft_pfa(P, L, lane); }
}

template <int IL> __device__ __forceinline__ float ltpf_s1(const float (&b)[12], const float* xb, int i)
{ float s = 0;
#pragma unroll
  for (int j = 0; j < IL - 1; j++) s += b[j] * xb[i - j];
  return s; }
template <int IL> __device__ __forceinline__ float ltpf_s2(const float (&a)[12], const float* yb, int i, int p)
{ float s = 0; const int i0 = i - p + IL / 2 - 1;
#pragma unroll
  for (int j = 0; j < IL; j++) s += a[j] * yb[i0 - j];
  return s; }
/* the filter loops for one tap-count class: IL = interpolation filter length (4, 6, 8, 12), tilt filter IL - 1 taps */
template <int IL> __device__ __forceinline__ void ltpf_core(SynLds& L, int lane, int N, int N4, int Lx, int Ly, int BS, int mode, int p1v, int p1, int p2,
                                                            const float (&a1)[12], const float (&a2)[12], const float (&b1)[12], const float (&b2)[12])
{
    constexpr int tilt_len = IL - 2;
    float* xb = L.A - Lx; float* yb = L.ly;
    const float fN4 = (float)N4;
    const int N34 = N - N4;
    /* first quarter (cross-fade) */
    for (int n0 = 0; n0 < N4; n0 += BS) {
        const int n = n0 + lane;
        if (lane < BS && n < N4) {
            const float xv = xb[Lx + n];
            float y;
            if (mode == 0) y = xv;
            else if (mode == 1 || mode == 4) { const float w = (fN4 - (float)n) / fN4; y = xv - w * ltpf_s1<IL>(b1, xb, Lx + n) + w * ltpf_s2<IL>(a1, yb, Ly + n, p1); }
            else if (mode == 2) { const float w = (float)n / fN4; y = xv - w * ltpf_s1<IL>(b2, xb, Lx + n) + w * ltpf_s2<IL>(a2, yb, Ly + n, p2); }
            else y = xv - ltpf_s1<IL>(b2, xb, Lx + n) + ltpf_s2<IL>(a2, yb, Ly + n, p2);
            yb[Ly + n] = y;
        }
        LSYNC();
    }
    if (mode == 4) {
        float* zb = L.sc;                        /* buf_z around the frame start: z[i] = buf_y[Ly - tilt_len + i], i < tilt_len + N4 (<= 130) */
        for (int i = lane; i < tilt_len + N4; i += WAVE) zb[i] = yb[Ly - tilt_len + i];
        LSYNC();
        for (int n0 = 0; n0 < N4; n0 += BS) {
            const int n = n0 + lane;
            if (lane < BS && n < N4) {
                const float w = (float)n / fN4;
                const float y = zb[tilt_len + n] - w * ltpf_s1<IL>(b2, zb, tilt_len + n) + w * ltpf_s2<IL>(a2, yb, Ly + n, p2);
                yb[Ly + n] = y;
            }
            LSYNC();
        }
    }
    /* remaining three quarters */
    if (p1v == 0) { for (int n = N4 + lane; n < N; n += WAVE) yb[Ly + n] = xb[Lx + n]; LSYNC(); }
    else for (int n0 = 0; n0 < N34; n0 += BS) {
        const int n = N4 + n0 + lane;
        if (lane < BS && n < N) yb[Ly + n] = xb[Lx + n] - ltpf_s1<IL>(b2, xb, Lx + n) + ltpf_s2<IL>(a2, yb, Ly + n, p2);
        LSYNC();
    }
}
/* In: the frame in L.A (behind its input history); returns where the frame's output samples are. */
__device__ __noinline__ const float* dec_ltpf(const lc3d_plan* __restrict__ P, SynLds& L, int lane, int bfi)
{
    const int fs = DPI(fs), N = DPI(N);
    int* st = L.st;
    int p0 = uni(L.isc[30]), p1v = uni(L.isc[31]), p2v = uni(L.isc[32]);
    int pitch_int = 0, pitch_fr = 0;
    float gain = 0;
    const float beta = __int_as_float(uni(L.isc[PR_LTPF])); const int beta_idx = uni(L.isc[PR_LTPF + 1]);      /* this frame's configuration (wave-uniform: one channel-stream) */
    if (bfi == 1) { p0 = 0; p1v = 0; }
    if (bfi != 1) {
        if (p0 == 1) {
            if (p2v < (127 - 32) * 4) { pitch_int = 32 + p2v / 4; pitch_fr = p2v - ((pitch_int - 32) * 4); }
            else if (p2v < ((127 - 32) * 4) + ((157 - 127) * 2)) { p2v = p2v - ((127 - 32) * 4); pitch_int = 127 + p2v / 2; pitch_fr = p2v - ((pitch_int - 127) * 2); pitch_fr = pitch_fr * 2; }
            else { pitch_int = p2v + (157 - ((127 - 32) * 4) - ((157 - 127) * 2)); pitch_fr = 0; }
            float pitch = (float)(((double)(float)pitch_int + (double)(float)pitch_fr / 4.0) * (double)(float)fs / 12800.0);
            pitch = (float)(round((double)pitch * 4.0) / 4.0);
            pitch_int = (int)floor((double)pitch);
            pitch_fr = (int)((double)(pitch - (float)pitch_int) * 4.0);
        }
        if (beta_idx < 0) p1v = 0;
        gain = p1v == 1 ? beta : 0.0f;
    }
    const int m1 = uni(st[DS_PARAM1]);
#ifndef LC3_BIG
    if (beta > 0) {
        const int cls = (fs == 8000 || fs == 16000) ? 0 : fs == 24000 ? 1 : fs == 32000 ? 2 : 3;
        const int inter_len_r = cls == 0 ? 4 : cls == 1 ? 6 : cls == 2 ? 8 : 12, tilt_len = inter_len_r - 2;
        const int inter_len = imax(fs, 16000) / 8000;
        const int Lx = tilt_len, Ly = (228 * fs / 12800) + inter_len;
        const int N4 = (int)((double)fs * 0.0025);
        float* xb = L.A - Lx; float* yb = L.ly;
        const int mode = (m1 == 0 && p1v == 0) ? 0 : (m1 == 1 && p1v == 0) ? 1 : (m1 == 0 && p1v == 1) ? 2
                       : (uni(st[DS_PITCH_INT]) == pitch_int && uni(st[DS_PITCH_FR]) == pitch_fr) ? 3 : 4;
        if (mode == 0) {
            /* neither this frame nor the previous one is filtered: the output is the input; only the histories move */
            for (int n = lane; n < N; n += WAVE) yb[Ly + n] = xb[Lx + n];
            LSYNC();
        } else {
            float a1[12], a2[12], b1[12], b2[12];
            const float mg = unif(__int_as_float(st[DS_GAIN]));
            const int mfr = uni(st[DS_PITCH_FR]), mbi = uni(st[DS_BETA_IDX]), pm1 = uni(st[DS_PITCH_INT]);
            int p1 = 0, p2 = 0;
#pragma unroll
            for (int i = 0; i < 12; i++) { a1[i] = a2[i] = b1[i] = b2[i] = 0; }
            if (m1 == 1) {
#pragma unroll
                for (int i = 0; i < 12; i++) { if (i < inter_len_r) a1[i] = mg * lc3t_ltpf_dec_inter[(cls * 4 + mfr) * 12 + i];
                                                if (i < inter_len_r - 1) b1[i] = (float)(0.85) * mg * lc3t_ltpf_dec_tilt[(cls * 4 + mbi) * 12 + i]; }
                p1 = pm1;
            }
            if (p1v == 1) {
#pragma unroll
                for (int i = 0; i < 12; i++) { if (i < inter_len_r - 1) b2[i] = (float)(0.85) * gain * lc3t_ltpf_dec_tilt[(cls * 4 + beta_idx) * 12 + i];
                                                if (i < inter_len_r) a2[i] = gain * lc3t_ltpf_dec_inter[(cls * 4 + pitch_fr) * 12 + i]; }
                p2 = pitch_int;
            }
            LSYNC();
            /* block size: the largest power of two <= the shortest feedback distance (p - inter_len + 1) of the filters in use */
            int lagmin = 64;
            if (m1 == 1) lagmin = imin(lagmin, p1 - inter_len + 1);
            if (p1v == 1) lagmin = imin(lagmin, p2 - inter_len + 1);
            int BS = 64; while (BS > lagmin && BS > 1) BS >>= 1;
            if (cls == 3) ltpf_core<12>(L, lane, N, N4, Lx, Ly, BS, mode, p1v, p1, p2, a1, a2, b1, b2);
            else if (cls == 2) ltpf_core<8>(L, lane, N, N4, Lx, Ly, BS, mode, p1v, p1, p2, a1, a2, b1, b2);
            else if (cls == 1) ltpf_core<6>(L, lane, N, N4, Lx, Ly, BS, mode, p1v, p1, p2, a1, a2, b1, b2);
            else ltpf_core<4>(L, lane, N, N4, Lx, Ly, BS, mode, p1v, p1, p2, a1, a2, b1, b2);
        }
        /* histories: buf[N .. N + len) -> buf[0 .. len), through registers (one barrier) */
        const float kx = lane < Lx ? xb[N + lane] : 0.0f;
        float ky[14];
#pragma unroll
        for (int r = 0; r < 14; r++) { const int i = lane + WAVE * r; ky[r] = i < Ly ? yb[N + i] : 0.0f; }
        LSYNC();
        if (lane < Lx) xb[lane] = kx;
#pragma unroll
        for (int r = 0; r < 14; r++) { const int i = lane + WAVE * r; if (i < Ly) yb[i] = ky[r]; }
    }
#else
    (void)m1; (void)beta;
#endif
    if (lane == 0) {
        st[DS_PARAM0] = p0; st[DS_PARAM1] = p1v; st[DS_PARAM2] = p2v;
        st[DS_PITCH_INT] = pitch_int; st[DS_PITCH_FR] = pitch_fr; st[DS_GAIN] = __float_as_int(gain); st[DS_BETA_IDX] = beta_idx;
    }
    LSYNC();
#ifndef LC3_BIG
    if (beta > 0) return &L.ly[(228 * fs / 12800) + imax(fs, 16000) / 8000];
#endif
    return L.A;
}

/* ------------------------------------------------------------------------------------------------ */
#if !defined(LC3_BIG) && !defined(LC3_PCM_PLACED)
/* Concealment bookkeeping: one channel-stream per lane, frames in order.  nbLostCmpt, the cumulative attenuation and the sign
 * generator's seed (R/plc_main.c, R/plc_noise_substitution0.c:13-40, R/plc_update.c:13-30) depend only on which frames are bad; a
 * lost frame gets (count, attenuation, first seed, index of the last good frame of this launch or -1) into its record.
 * Every frame also gets its LTPF configuration (PR_LTPF): the channel's configuration, or with per-frame sizes (0 = lost) that of the frame's
 * size, a lost frame keeping the one of the last good frame (R/dec_lc3_fl.c:146-155) - the channel's configuration before the call at first. */
/* _rag: a lane's frames end at its stream's count; the lanes of a wave end at different frames, so the wave walks to the largest count among them and a lane
 * past its own takes no part (it is not `live`: never lost, so the seed loop under __any leaves its seed alone).  The scalars are written back from the
 * count's frame; with count 0 nothing is written. */
extern "C" __global__ void __launch_bounds__(WAVE)
DEC_RAG(lc3_dec_plc_kernel)(const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ chans, const uint16_t* __restrict__ sizes /* [stream][T] or null */,
                   const lc3d_dchan* __restrict__ dtab, float* __restrict__ state, int* __restrict__ rec, int T, int ncs LC3_RAGGED_OPT)
{
    const int cs = blockIdx.x * WAVE + threadIdx.x;
    const bool valid = cs < ncs;
    const int Lspec = P->ylen, channels = P->channels, strm = cs / channels, ch = cs % channels;
    float beta = valid ? chans[cs].ltpf_beta : 0.0f; int beta_idx = valid ? chans[cs].ltpf_beta_idx : -1;
    int* sc = (int*)(state + (size_t)(valid ? cs : 0) * DST_WORDS + DST_SCAL);
    int nbl = valid ? sc[DS_NBLOST] : 0, seed = valid ? sc[DS_PLC_SEED] : 0, prev = valid ? sc[DS_PREV_BFI] : 0, pprev = valid ? sc[DS_PREVPREV_BFI] : 0;
    float ca = valid ? __int_as_float(sc[DS_CUM_ALPHA]) : 1.0f;
    int last_good = -1;
#ifdef LC3_DEC_RAGGED
    const int Tc = valid ? DEC_TC(strm) : 0;
    int Tw = Tc;
    for (int o = WAVE / 2; o > 0; o >>= 1) Tw = imax(Tw, __shfl_xor(Tw, o));
#define PLC_END Tw
#define PLC_LIVE(t_) (valid && (t_) < Tc)
#else                                    /* the dense kernel's tokens, so that it stays the code it was */
#define PLC_END T
#define PLC_LIVE(t_) valid
#endif
    for (int t = 0; t < PLC_END; t++) {
        int* r = rec + ((size_t)(valid ? cs : 0) * T + t) * PR_WORDS;
        const int bfi = PLC_LIVE(t) ? r[PR_BFI] : 0;
        const bool lost = PLC_LIVE(t) && bfi == 1;
        if (PLC_LIVE(t)) {
            const int fsz = sizes ? (int)sizes[(size_t)strm * T + t] : 0;
            if (fsz) { const lc3d_dchan* d = &dtab[fsz / channels + (ch < fsz % channels)]; beta = d->ltpf_beta; beta_idx = d->ltpf_beta_idx; }
            r[PR_LTPF] = __float_as_int(beta); r[PR_LTPF + 1] = beta_idx;
        }
        if (lost) {
            nbl = nbl + 1;
            const float alpha = nbl < 4 ? 1.0f : nbl < 8 ? (float)0.9 : (float)0.85;
            ca = ca * alpha;
            r[PR_PLC + 0] = nbl; r[PR_PLC + 1] = __float_as_int(ca); r[PR_PLC + 2] = seed; r[PR_PLC + 3] = last_good;
        }
        if (__any(lost)) {
            for (int j = 0; j < Lspec; j++) {            /* the generator runs once per spectral line of a lost frame */
                int s2 = 16831 + seed * 12821;
                s2 = (int)((double)s2 - round((double)((float)s2 * 0x1p-16f)) * (double)0x1p16f);
                if (s2 == 32768) s2 -= 32768;
                if (lost) seed = s2;
            }
        }
        if (PLC_LIVE(t) && !lost) { last_good = t; nbl = 0; ca = 1.0f; }
#ifdef LC3_DEC_RAGGED
        if (PLC_LIVE(t)) { pprev = prev; prev = bfi; }
#else
        pprev = prev; prev = bfi;
#endif
    }
    if (PLC_LIVE(0)) { sc[DS_NBLOST] = nbl; sc[DS_CUM_ALPHA] = __float_as_int(ca); sc[DS_PLC_SEED] = seed; sc[DS_PREV_BFI] = prev; sc[DS_PREVPREV_BFI] = pprev; }
#undef PLC_LIVE
#undef PLC_END
}

#ifndef LC3_DEC_RAGGED
/* Per-frame sizes and flags in device memory (lc3plus_dec_batch_decode_sizes_device), before the parser: one stream-frame per lane, the rule of
 * lc3d_dec_frame_class (lc3_plan.h).  Writes what the per-frame-size kernels take - the size of every good frame and 0 where the frame is lost, and the
 * lost flag - and marks the frames lost because their size or flag is invalid. */
extern "C" __global__ void __launch_bounds__(256)
lc3_dec_plan_sizes_kernel(const int32_t* __restrict__ num_bytes, const uint8_t* __restrict__ bfi /* or null */, const lc3d_dchan* __restrict__ dtab,
                          int tab_n, int channels, int in_stride, long long n, uint16_t* __restrict__ sizes, uint8_t* __restrict__ lost,
                          uint8_t* __restrict__ invalid)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int nb = num_bytes[i];
    const int k = lc3d_dec_frame_class(nb, bfi ? (int)bfi[i] : 0, in_stride, dtab, tab_n, channels);
    sizes[i] = k == LC3D_FRAME_GOOD ? (uint16_t)nb : (uint16_t)0;
    lost[i] = k != LC3D_FRAME_GOOD;
    invalid[i] = k >= LC3D_FRAME_BAD_FLAG;
}

/* The same for frames packed back to back (lc3plus_dec_batch_decode_packed): the rule of lc3d_dec_frame_class_packed, with each frame's offset and the
 * caller's capacity in place of in_stride.  A frame that breaks it is invalid like a bad size: it is never read and does not move the carry. */
extern "C" __global__ void __launch_bounds__(256)
lc3_dec_plan_packed_kernel(const int32_t* __restrict__ num_bytes, const long long* __restrict__ offs, const uint8_t* __restrict__ bfi /* or null */,
                           const lc3d_dchan* __restrict__ dtab, int tab_n, int channels, long long cap, int max_bytes, long long n, uint16_t* __restrict__ sizes,
                           uint8_t* __restrict__ lost, uint8_t* __restrict__ invalid)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int nb = num_bytes[i], fl = bfi ? (int)bfi[i] : 0;
    const long long off = (fl == 0 && nb != 0) ? offs[i] : 0;        /* a lost frame's offset is not looked at */
    const int k = lc3d_dec_frame_class_packed(nb, fl, off, cap, max_bytes, dtab, tab_n, channels);
    sizes[i] = k == LC3D_FRAME_GOOD ? (uint16_t)nb : (uint16_t)0;
    lost[i] = k != LC3D_FRAME_GOOD;
    invalid[i] = k >= LC3D_FRAME_BAD_FLAG;
}

/* ... and after the synthesis: one stream-frame per lane.  An invalid frame's status gets LC3D_DEC_ST_INVALID beside the concealment bit the synthesis
 * wrote.  The lane of a stream's last frame configures the stream with the size of its last good frame of the call (the configuration stays when the
 * call has none): every channel from dtab, with its payload offset, as lc3plus_dec_batch_decode_sizes does on the host.  The concealment kernel of the
 * next call starts its LTPF carry from there, and a later fixed-size parser reads it. */
extern "C" __global__ void __launch_bounds__(256)
lc3_dec_sizes_tail_kernel(const uint16_t* __restrict__ sizes, const uint8_t* __restrict__ invalid, const lc3d_dchan* __restrict__ dtab, int channels,
                          int n_streams, int T, lc3d_dchan* __restrict__ chans, uint8_t* __restrict__ status /* [stream][T] or null */)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n_streams * T) return;
    if (status && invalid[i]) status[i] |= LC3D_DEC_ST_INVALID;
    if (i % T != T - 1) return;
    const long long s = i / T;
    const uint16_t* z = sizes + s * T;
    int t = T - 1;
    while (t >= 0 && z[t] == 0) t--;
    if (t < 0) return;
    const int fsz = z[t];
    for (int c = 0, off = 0; c < channels; c++) {
        lc3d_dchan d = dtab[fsz / channels + (c < fsz % channels)];
        d.in_off = off; off += d.nbytes;
        chans[s * channels + c] = d;
    }
}
#else /* LC3_DEC_RAGGED */
/* The three kernels above with per-stream frame counts.  The plan kernels clamp the caller's count into cnt [stream] (the lane of a stream's first frame writes it;
 * every later kernel of the call reads that copy) and give an absent frame - t >= count - size 0, lost 1, invalid 0 without reading any of its entries: that is
 * what the per-frame-size parser takes for a frame it stages and reads nothing of, so the parser has no ragged form. */
extern "C" __global__ void __launch_bounds__(256)
lc3_dec_plan_sizes_kernel_rag(const int32_t* __restrict__ num_bytes, const uint8_t* __restrict__ bfi /* or null */, const lc3d_dchan* __restrict__ dtab,
                              int tab_n, int channels, int in_stride, long long n, uint16_t* __restrict__ sizes, uint8_t* __restrict__ lost,
                              uint8_t* __restrict__ invalid, const int32_t* __restrict__ counts, int T, int32_t* __restrict__ cnt)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = (int)(i % T), c = lc3d_dec_count_clamp(counts[i / T], T);
    if (t == 0) cnt[i / T] = c;
    if (t >= c) { sizes[i] = 0; lost[i] = 1; invalid[i] = 0; return; }
    const int nb = num_bytes[i];
    const int k = lc3d_dec_frame_class(nb, bfi ? (int)bfi[i] : 0, in_stride, dtab, tab_n, channels);
    sizes[i] = k == LC3D_FRAME_GOOD ? (uint16_t)nb : (uint16_t)0;
    lost[i] = k != LC3D_FRAME_GOOD;
    invalid[i] = k >= LC3D_FRAME_BAD_FLAG;
}
extern "C" __global__ void __launch_bounds__(256)
lc3_dec_plan_packed_kernel_rag(const int32_t* __restrict__ num_bytes, const long long* __restrict__ offs, const uint8_t* __restrict__ bfi /* or null */,
                               const lc3d_dchan* __restrict__ dtab, int tab_n, int channels, long long cap, int max_bytes, long long n, uint16_t* __restrict__ sizes,
                               uint8_t* __restrict__ lost, uint8_t* __restrict__ invalid, const int32_t* __restrict__ counts, int T, int32_t* __restrict__ cnt)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = (int)(i % T), c = lc3d_dec_count_clamp(counts[i / T], T);
    if (t == 0) cnt[i / T] = c;
    if (t >= c) { sizes[i] = 0; lost[i] = 1; invalid[i] = 0; return; }
    const int nb = num_bytes[i], fl = bfi ? (int)bfi[i] : 0;
    const long long off = (fl == 0 && nb != 0) ? offs[i] : 0;        /* a lost frame's offset is not looked at */
    const int k = lc3d_dec_frame_class_packed(nb, fl, off, cap, max_bytes, dtab, tab_n, channels);
    sizes[i] = k == LC3D_FRAME_GOOD ? (uint16_t)nb : (uint16_t)0;
    lost[i] = k != LC3D_FRAME_GOOD;
    invalid[i] = k >= LC3D_FRAME_BAD_FLAG;
}
/* ... and behind the synthesis.  An absent frame's status is LC3D_DEC_ST_ABSENT by store - no kernel of the call has written it, and the caller's buffer is not
 * initialised - and neither the invalid bit nor the placement bit looks at it; a present frame gets both as in the dense call (plo null: no placement; the marking
 * of lc3_pcm_placed_mark_kernel is done here, it would OR into the absent frames).  The last good size is searched among the present frames. */
extern "C" __global__ void __launch_bounds__(256)
lc3_dec_sizes_tail_kernel_rag(const uint16_t* __restrict__ sizes, const uint8_t* __restrict__ invalid, const lc3d_dchan* __restrict__ dtab, int channels,
                              int n_streams, int T, lc3d_dchan* __restrict__ chans, uint8_t* __restrict__ status /* [stream][T] or null */,
                              const int32_t* __restrict__ cnt, const long long* __restrict__ plo /* or null */, long long plcap, int N)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n_streams * T) return;
    const long long s = i / T;
    const int c = cnt[s];
    if (status) {
        if (i % T >= c) status[i] = LC3D_DEC_ST_ABSENT;
        else {
            int b = invalid[i] ? LC3D_DEC_ST_INVALID : 0;
            if (plo && !lc3d_pcm_placed_ok(plo[i], channels, N, plcap)) b |= LC3D_DEC_ST_PCM_PLACE;
            if (b) status[i] |= (uint8_t)b;
        }
    }
    if (i % T != T - 1) return;
    const uint16_t* z = sizes + s * T;
    int t = c - 1;
    while (t >= 0 && z[t] == 0) t--;
    if (t < 0) return;
    const int fsz = z[t];
    for (int k = 0, off = 0; k < channels; k++) {
        lc3d_dchan d = dtab[fsz / channels + (k < fsz % channels)];
        d.in_off = off; off += d.nbytes;
        chans[s * channels + k] = d;
    }
}
#endif /* LC3_DEC_RAGGED */
#endif

#ifndef LC3_PCM_PLACED
/* ------------------------------------------------------------------------------------------------ */
/* A run of IMDCT_FPW consecutive frames of one channel-stream per wave, every frame on its own: shaped (or concealed) spectrum ->
 * DCT-IV -> window.  The overlap-add needs the previous frame and is left to the synthesis kernel: this kernel is stateless, all
 * runs of a launch are independent (ncs * ceil(T / IMDCT_FPW) waves).  The hand-over of the next frame is fetched during the transform. */
extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(DEC_IMDCT_WAVES, DEC_IMDCT_WAVES)))
DEC_IMDCT_KERNEL(const lc3d_plan* __restrict__ P, const float* __restrict__ state, const int* __restrict__ rec /* [cs][T][PR_WORDS] */,
                 const float* __restrict__ ws /* [cs][T][WS_ROW(N)] */, int T, int ncs, float* __restrict__ ov /* [cs][T][OV_ROW(N)] */,
                 lc3d_dec_trace* __restrict__ trace LC3_RAGGED_OPT)
{
    __shared__ ImdLds L;
    const int lane = threadIdx.x;
    const int runs = (T + IMDCT_FPW - 1) / IMDCT_FPW;
    const int cs = blockIdx.x / runs, t0 = (blockIdx.x % runs) * IMDCT_FPW;
    if (cs >= ncs) return;
    const int t1 = imin(DEC_TC(cs / P->channels), t0 + IMDCT_FPW);
#ifdef LC3_DEC_RAGGED
    if (t0 >= t1) return;                            /* a run wholly past the stream's count; one that straddles it stops there (t1) */
#endif
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    LSYNC();
    const int N = DPI(N), Lspec = DPI(ylen), la = DPI(la), h = N >> 1, wsr = WS_ROW(N);
    int* isc = L.isc;
    float* X = XCUR(L);
    const float norm = DPF(dct4_norm);
    {
        const int nb = DPI(nbands), lim = lc3t_band_pool[DPI(band_off) + nb];
        for (int j = lane; j < MAXN; j += WAVE) {
            const int b = j < N ? (int)P->band_of_bin[j] : 255;
            L.bsel[j] = (unsigned char)((b < nb && j < lim) ? b : 255);
        }
    }
    /* LDS-DMA: 64 lanes x 4 bytes land at base + 4 * lane (global_load_lds_dword); nothing passes through registers, so no value is
     * live across the transform's calls.  The next LSYNC waits for it (hipcc drains the VM counter at a barrier). */
#define PREFETCH(tt_) do { \
        const int* r_ = rec + ((size_t)cs * T + (tt_)) * PR_WORDS; const float* row_ = LC3D_ROW_BASE(ws, cs, (tt_), T, wsr); \
        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(r_ + lane), (void __attribute__((address_space(3)))*)L.isc, 4, 0, 0); \
        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(r_ + PR_GAINS + lane), (void __attribute__((address_space(3)))*)L.gi, 4, 0, 0); \
        for (int k_ = 0; k_ < NR; k_++) if (WAVE * k_ + lane < Lspec)   /* inactive lanes neither read nor write */ \
            __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(row_ + LC3D_ROW_OFF(WAVE * k_ + lane, T)), (void __attribute__((address_space(3)))*)&L.nrow[WAVE * k_], 4, 0, 0); \
    } while (0)
    PREFETCH(t0);
    LSYNC();
    const int lane0 = lane;
    for (int t = t0; t < t1; t++) {
        int lane = lane0;
        asm volatile("" : "+v"(lane));             /* keeps per-lane address arithmetic inside the iteration: hoisted, it would be spilled around the transform's calls */
        const size_t cf = (size_t)cs * T + t;
        lc3d_dec_trace* tr = trace ? &trace[cf] : nullptr;
        LSYNC();                                      /* the hand-over of this frame has landed */
        const int bfi = uni(isc[PR_BFI]);
        if (bfi != 1) {
            if (tr) {
                if (lane == 0) { tr->bw_idx = isc[0]; tr->lastnz = isc[1]; tr->lsb_mode = isc[2]; tr->gg_idx = isc[3]; tr->fac_ns = isc[33]; tr->nfilt = isc[4];
                                 tr->tns_order[0] = isc[5]; tr->tns_order[1] = isc[6]; tr->nf_seed = isc[37]; tr->zero_frame = isc[38]; tr->nres = isc[34];
                                 for (int i = 0; i < 3; i++) tr->ltpf[i] = isc[30 + i]; for (int i = 0; i < 7; i++) tr->scf_idx[i] = isc[23 + i]; }
                if (lane < 16) tr->tns_idx[lane] = isc[7 + lane];
#pragma unroll
                for (int k = 0; k < NR; k++) { const int j = lane + WAVE * k; if (j < Lspec) tr->q_tns[j] = L.nrow[j]; }
            }
            /* ---- SNS shaping R/mdct_shaping.c with the band gains of the parse kernel ---- */
#pragma unroll
            for (int k = 0; k < NR; k++) {
                const int j = lane + WAVE * k;
                if (j < MAXN) {
                    float v = j < Lspec ? L.nrow[j] : 0.0f;
                    const int b = L.bsel[j];
                    if (b != 255) v = v * L.gi[b];
                    L.A[j] = v;
                }
            }
        } else {
            /* ---- concealment R/plc_noise_substitution0.c: the last good spectrum with random signs, fading ---- */
            const int src = uni(isc[PR_PLC + 3]);
            const float ca = __int_as_float(uni(isc[PR_PLC + 1]));
            int seed = uni(isc[PR_PLC + 2]);
            float prev[NR];
            if (src >= 0) {                           /* rebuilt from the hand-over of that frame: same products as when it was decoded */
                const float* rowg = LC3D_ROW_BASE(ws, cs, src, T, wsr);
                LSYNC();
                L.gi[lane] = __int_as_float(rec[((size_t)cs * T + src) * PR_WORDS + PR_GAINS + lane]);
                LSYNC();
#pragma unroll
                for (int k = 0; k < NR; k++) {
                    const int j = lane + WAVE * k;
                    float v = j < Lspec ? rowg[LC3D_ROW_OFF(j, T)] : 0.0f;
                    const int b = j < MAXN ? (int)L.bsel[j] : 255;
                    if (b != 255) v = v * L.gi[b];
                    prev[k] = v;
                }
            } else {
#pragma unroll
                for (int k = 0; k < NR; k++) { const int j = lane + WAVE * k; prev[k] = j < Lspec ? state[(size_t)cs * DST_WORDS + DST_QPREV + j] : 0.0f; }
            }
#pragma unroll
            for (int k = 0; k < NR; k++) {
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
                if (i0 + lane < MAXN) L.A[i0 + lane] = i0 + lane < Lspec ? prev[k] * mine : 0.0f;
            }
        }
        LSYNC();
        if (t + 1 < t1) PREFETCH(t + 1);              /* isc, gi and the spectrum registers of this frame have been consumed */
        if (tr) { if (lane == 0) tr->bfi = bfi; for (int i = lane; i < Lspec; i += WAVE) tr->q_shaped[i] = L.A[i]; }
        /* ---- IMDCT R/imdct.c:13-59 ---- */
#pragma unroll
        for (int k = 0; k < NH; k++) {                          /* pre-twiddle R/dct4.c:84-86: A -> X */
            const int i = lane + WAVE * k;
            if (i < h) {
                const float ar = L.A[2 * i], ai = L.A[N - 2 * i - 1], br = P->tw1[2 * i], bi = P->tw1[2 * i + 1];
                X[2 * i] = ar * br - ai * bi; X[2 * i + 1] = ai * br + ar * bi;
            }
        }
        LSYNC();
        dec_dft(P, L, lane);                                   /* X -> A */
        float pr[NH], pi[NH];                                  /* post-twiddle R/dct4.c:90-94, in place: A -> time-domain aliasing buffer */
#pragma unroll
        for (int k = 0; k < NH; k++) {
            const int i = lane + WAVE * k;
            pr[k] = 0; pi[k] = 0;
            if (i < h) {
                const float ar = L.A[2 * i], ai = L.A[2 * i + 1], br = P->tw2[2 * i], bi = P->tw2[2 * i + 1];
                const float trr = ar * br - ai * bi, ti = ai * br + ar * bi;
                pr[k] = trr * norm; pi[k] = -ti * norm;
            }
        }
        LSYNC();
        float* tda = L.A;
#pragma unroll
        for (int k = 0; k < NH; k++) { const int i = lane + WAVE * k; if (i < h) { tda[2 * i] = pr[k]; tda[N - 2 * i - 1] = pi[k]; } }
        LSYNC();
        /* the window and the overlap-add belong to the synthesis kernel: it reads this buffer through the fold pattern of R/imdct.c:34-58 */
        float* o = ov + cf * OV_ROW(N);
        for (int n = lane; n < N; n += WAVE) o[n] = tda[n];
        LSYNC();
    }
#undef PREFETCH
}
#endif /* !LC3_PCM_PLACED */

/* ------------------------------------------------------------------------------------------------ */
/* One channel-stream per wave, frames in order: overlap-add, LTPF synthesis, output.  The overlap memory lives in registers. */
#ifndef DEC_SYNTH_EU
#define DEC_SYNTH_EU 4
#endif
extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(DEC_SYNTH_EU, DEC_SYNTH_EU)))
DEC_SYNTH_KERNEL(const lc3d_plan* __restrict__ P, float* __restrict__ state,
                 const int* __restrict__ rec, const float* __restrict__ ws, const float* __restrict__ ov /* [cs][T][OV_ROW(N)] */, int T,
                 void* __restrict__ pcm, int bps, int ncs, uint8_t* __restrict__ status /* [stream][T] or null */, lc3d_dec_trace* __restrict__ trace LC3_PLACED_OPT LC3_RAGGED_OPT)
{
    __shared__ SynLds L;
    const int lane = threadIdx.x, cs = blockIdx.x;
    if (cs >= ncs) return;
    const int Tc = DEC_TC(cs / P->channels);         /* the frames of this stream in the call: T, or with _rag the stream's count */
#ifdef LC3_DEC_RAGGED
    if (Tc <= 0) return;                              /* no present frame: the state rows stay untouched */
#endif
    if (lane < LC3D_PLAN_HEAD_WORDS) L.pc[lane] = ((const int*)P)[lane];
    float* stp = state + (size_t)cs * DST_WORDS;
#ifndef LC3_BIG
    for (int i = lane; i < DEC_LY; i += WAVE) L.ly[i] = stp[DST_LY + i];
#endif
    if (lane < DEC_LX) L.lxh[lane] = stp[DST_LX + lane];
    if (lane < 16) L.st[lane] = ((const int*)stp)[DST_SCAL + lane];
    LSYNC();
    const int N = DPI(N), Lspec = DPI(ylen), channels = DPI(channels), la = DPI(la), ovr = OV_ROW(N);
    const int strm = cs / channels, ch = cs % channels;
    const int h = N >> 1;
    float mem[NM];                                    /* IMDCT overlap memory of samples lane + 64 k */
    float wo[NR], wm[NM];                             /* window taps of the output samples lane + 64 k and of the new overlap memory (R/imdct.c) */
    {
        const float* w = &lc3t_win_pool[DPI(win_off)];
#pragma unroll
        for (int k = 0; k < NM; k++) { const int j = lane + WAVE * k; mem[k] = j < N - la ? stp[DST_IMEM + j] : 0.0f; wm[k] = j < N - la ? w[N - 1 - la - j] : 0.0f; }
#pragma unroll
        for (int k = 0; k < NR; k++) { const int j = lane + WAVE * k; wo[k] = j < N ? w[2 * N - 1 - (la + j)] : 0.0f; }
    }
    /* x_ov[i], i < 2N: [tda[h..N) | -tda[N-1..h] | -tda[h-1..0] | -tda[0..h)] * win[2N-1-i]; out = x_ov[la..la+N) (+ memory), memory = x_ov[N+la..2N) */
#define XOVI(i_) ((i_) < h ? h + (i_) : (i_) < N ? N - 1 - ((i_) - h) : (i_) < N + h ? h - 1 - ((i_) - N) : (i_) - N - h)

    /* ---- the hand-over of frame t + 1 is fetched while frame t is being synthesised: unconditional loads from clamped indices (a `cond ? load : 0`
     *      is a select on the loaded register and waits for the load on the spot - thirteen serialised round trips per frame); the lanes past the frame's end
     *      hold a copy of its last sample, which nothing uses (their stores are masked, their window taps are zero) ---- */
    int pf_isc = 0; float pf_out[NR], pf_mem[NM];
#define PREFETCH(tt_) do { \
        const int* r_ = rec + ((size_t)cs * T + (tt_)) * PR_WORDS; const float* o_ = ov + ((size_t)cs * T + (tt_)) * ovr; \
        pf_isc = r_[imin(lane, 47)]; \
        _Pragma("unroll") for (int k = 0; k < NR; k++) { const int j = imin(lane + WAVE * k, N - 1); pf_out[k] = o_[XOVI(la + j)]; } \
        _Pragma("unroll") for (int k = 0; k < NM; k++) { const int j = imin(lane + WAVE * k, N - la - 1); pf_mem[k] = o_[XOVI(N + la + j)]; } } while (0)
    PREFETCH(0);
    int last_good = -1;

#ifdef LC3_STAGE_TIMING
    if (lane < 16) L.tacc[lane] = 0;
    LSYNC();
    long long tlast = clock64();
#endif
    const int lane0 = lane;
    for (int t = 0; t < Tc; t++) {
        int lane = lane0;
        asm volatile("" : "+v"(lane));             /* keeps per-lane address arithmetic inside the iteration instead of in spilled registers */
#ifdef LC3_STAGE_TIMING
        lc3d_dec_trace* tr = nullptr;
#else
        lc3d_dec_trace* tr = trace ? &trace[(size_t)cs * T + t] : nullptr;
#endif
        if (lane < 48) L.isc[lane] = pf_isc;
        /* ---- overlap-add R/imdct.c:50-58 ---- */
#pragma unroll
        for (int k = 0; k < NR; k++) {
            const int n = lane + WAVE * k;
            float v = (la + n < h ? pf_out[k] : -pf_out[k]) * wo[k];
            if (k < NM && n < N - la) v = v + mem[k < NM ? k : 0];
            if (n < N) L.A[n] = v;
        }
#pragma unroll
        for (int k = 0; k < NM; k++) mem[k] = -pf_mem[k] * wm[k];
        LSYNC();
        const int bfi = uni(L.isc[PR_BFI]);
        if (bfi != 1) last_good = t;
        if (t + 1 < Tc) PREFETCH(t + 1);
        DTICK(0);
        if (tr) for (int i = lane; i < N; i += WAVE) tr->x_imdct[i] = L.A[i];
        /* ---- LTPF synthesis R/ltpf_decoder.c:13-316 ---- */
        const float* out = dec_ltpf(P, L, lane, bfi);
        if (tr) for (int i = lane; i < N; i += WAVE) tr->x_out[i] = out[i];
        if (status && ch == channels - 1 && lane == 0) status[(size_t)strm * T + t] = (uint8_t)(bfi == 1);   /* R/dec_lc3_fl.c:162 */
        DTICK(9);
        /* ---- output R/dec_lc3_fl.c:115-127 ---- */
        {
            /* bps is the PCM format word (lc3_plan.h: lc3d_pcm_*): the sample type, and the layout that gives the frame's first element and the step between samples */
#ifdef LC3_PCM_PLACED
            const long long poff = plo[(size_t)strm * T + t];
            const bool pok = lc3d_pcm_placed_ok(poff, channels, N, plcap) != 0;                /* an invalid frame is decoded like any other and written nowhere */
            const size_t o = pok ? lc3d_pcm_placed_frame(bps, channels, N, poff, ch) : 0;
            const int ps = lc3d_pcm_stride(bps, channels), ty = bps & LC3D_PCM_TYPE_MASK;
            if (!pok) { }
            else
#else
            const size_t o = lc3d_pcm_frame(bps, channels, T, N, strm, t, ch);
            const int ps = lc3d_pcm_stride(bps, channels), ty = bps & LC3D_PCM_TYPE_MASK;
#endif
            if (ty == 16) {
                int16_t* op = (int16_t*)pcm + o;
                for (int i = lane; i < N; i += WAVE) {
                    const float tt = (float)round((double)(0x1p15f * (out[i] * 0x1p-15f)));
                    op[(size_t)i * ps] = (int16_t)fmaxf(fminf(tt, 32767.0f), -32768.0f);
                }
            } else if (ty == LC3D_PCM_FLOAT32) {
                /* float: the synthesised sample at full scale 1.0, neither rounded nor clipped; 16 bytes per lane where the samples follow each other */
                float* op = (float*)pcm + o;
                if (ps == 1 && (N & 3) == 0 && (((size_t)op) & 15) == 0) {
                    for (int i = lane; i < (N >> 2); i += WAVE)
                        ((float4*)op)[i] = make_float4(out[4 * i] * 0x1p-15f, out[4 * i + 1] * 0x1p-15f, out[4 * i + 2] * 0x1p-15f, out[4 * i + 3] * 0x1p-15f);
                } else for (int i = lane; i < N; i += WAVE) op[(size_t)i * ps] = out[i] * 0x1p-15f;
            } else if (lc3d_pcm_type_wire(ty)) {
                /* the wire types (lc3_plan.h): the 16- or 24-bit integer result of the branches around this one, then bytes swapped, saturated to 24 bits or
                 * compressed by G.711.  Exactly N elements of 1, 2 or 3 bytes are written: one, two or three whole dwords (four samples) per lane where the samples
                 * follow each other and the frame's first byte is on a dword, the rest byte by byte. */
                const int eb = lc3d_pcm_elem_bytes(ty);
                uint8_t* op = (uint8_t*)pcm + o * eb;
                const bool w24 = eb == 3, be = ty == LC3D_PCM_S16_BE || ty == LC3D_PCM_S24_3BE, al = ty == LC3D_PCM_ALAW;
                /* sample i as the bytes it is stored as, the first byte lowest */
                auto wire = [&](int i) -> unsigned {
                    if (w24) {
                        const double r = round((double)(0x1p23f * (out[i] * 0x1p-15f)));
                        const unsigned v = (unsigned)lc3d_pcm_sat24((r >= -2147483648.0 && r < 2147483648.0) ? (int32_t)r : (int32_t)0x80000000) & 0xffffffu;
                        return be ? __builtin_bswap32(v) >> 8 : v;
                    }
                    const float tt = (float)round((double)(0x1p15f * (out[i] * 0x1p-15f)));
                    const int x = (int)fmaxf(fminf(tt, 32767.0f), -32768.0f);
                    if (eb == 1) return (unsigned)lc3d_g711_compress(x, al);
                    return be ? __builtin_bswap32((unsigned)x) >> 16 : (unsigned)x & 0xffffu;
                };
                int done = 0;
                if (ps == 1 && (((size_t)op) & 3) == 0) {            /* four samples per lane, like the float output: 4, 8 or 12 bytes of whole dwords, consecutive lanes consecutive bytes */
                    for (int i = lane; i < (N >> 2); i += WAVE) {
                        const unsigned a = wire(4 * i), b = wire(4 * i + 1), c = wire(4 * i + 2), e = wire(4 * i + 3);
                        unsigned* q = (unsigned*)op + eb * i;
                        if (eb == 1) q[0] = a | b << 8 | c << 16 | e << 24;
                        else if (eb == 2) { q[0] = a | b << 16; q[1] = c | e << 16; }
                        else { q[0] = a | b << 24; q[1] = b >> 8 | c << 16; q[2] = c >> 16 | e << 8; }
                    }
                    done = N & ~3;
                }
                for (int i = done + lane; i < N; i += WAVE) {
                    const unsigned v = wire(i);
                    uint8_t* q = op + (size_t)i * ps * eb;
                    q[0] = (uint8_t)v;
                    if (eb > 1) q[1] = (uint8_t)(v >> 8);
                    if (eb > 2) q[2] = (uint8_t)(v >> 16);
                }
            } else {
                int32_t* op = (int32_t*)pcm + o;
                const float sc = ty == 24 ? 0x1p23f : 0x1p31f;
                for (int i = lane; i < N; i += WAVE) {
                    /* the reference converts without clipping (R/dec_lc3_fl.c:123-125); out of range that is undefined in C and yields
                     * INT32_MIN on the x86-64 builds the vectors come from (cvttsd2si), for either sign and for NaN: reproduced here */
                    const double r = round((double)(sc * (out[i] * 0x1p-15f)));
                    op[(size_t)i * ps] = (r >= -2147483648.0 && r < 2147483648.0) ? (int32_t)r : (int32_t)0x80000000;
                }
            }
        }
        LSYNC();
        DTICK(10);
    }
#undef PREFETCH
#undef XOVI
#ifdef LC3_STAGE_TIMING
    if (trace && lane < 16) ((long long*)&trace[(size_t)cs * T])[lane] = L.tacc[lane];
#endif
#pragma unroll
    for (int k = 0; k < NM; k++) { const int j = lane + WAVE * k; if (j < N - la) stp[DST_IMEM + j] = mem[k]; }
    if (last_good >= 0) {                             /* the spectrum a lost frame of the next launch would repeat */
        const int nb = DPI(nbands), lim = lc3t_band_pool[DPI(band_off) + nb], wsr = WS_ROW(N);
        const float* rowg = LC3D_ROW_BASE(ws, cs, last_good, T, wsr);
        LSYNC();
        L.sc[lane] = __int_as_float(rec[((size_t)cs * T + last_good) * PR_WORDS + PR_GAINS + lane]);
        LSYNC();
        for (int j = lane; j < Lspec; j += WAVE) {
            float v = rowg[LC3D_ROW_OFF(j, T)];
            const int b = (int)P->band_of_bin[j];
            if (b < nb && j < lim) v = v * L.sc[b];
            stp[DST_QPREV + j] = v;
        }
    }
#ifndef LC3_BIG
    for (int i = lane; i < DEC_LY; i += WAVE) stp[DST_LY + i] = L.ly[i];
#endif
    if (lane < DEC_LX) stp[DST_LX + lane] = L.lxh[lane];
    if (lane < 7) ((int*)stp)[DST_SCAL + lane] = L.st[lane];      /* the LTPF scalars; the concealment scalars belong to lc3_dec_plc_kernel */
}
