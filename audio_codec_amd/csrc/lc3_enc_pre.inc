/* lc3_enc_pre.inc -- the 12.8 kHz resampler and its HP50 filter ahead of lc3_encode_kernel (included by lc3_kernels.hip).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point, R/resamp12k8.c:13-80.  The polyphase FIR of a frame needs that frame's
 * PCM and the tail of the previous frame's - no encoder state - so lc3_enc_resample_kernel runs it for all B x T frames at once,
 * a run of frames per wave.  The HP50 biquad behind it is a strictly serial double-precision recurrence (128 steps of six operations
 * per frame): inside lc3_encode_kernel the whole wave executes it for one stream, about 12 % of that kernel's instruction time.
 * lc3_enc_hp50_kernel gives every stream a LANE and walks all frames of the launch; the filter state is rounded to float at each
 * frame boundary exactly as the frame-wise code does (R/setup_enc_lc3.h: r12k8_mem_50 is LC3_FLOAT). */

struct __attribute__((aligned(16))) PreLds {
    float xs[LC3D_MAX_N + 128];          /* [previous frame's tail (rs_mem_in_len) | this frame], scaled */
    float taps[240];                     /* the polyphase filter: from global memory every tap load would be waited for together with the next frame's PCM (vmcnt counts in issue order) */
    int pc[LC3D_PLAN_HEAD_WORDS];
};
#ifndef HP_WAVES
#define HP_WAVES 1
#endif

__device__ __forceinline__ float pre_pcm(const void* __restrict__ pcm, int bitdepth, size_t idx)   /* the encoder's input conversion (R/enc_lc3_fl.c:30-42) */
{
    if (bitdepth == 16) return (float)((const int16_t*)pcm)[idx];
    return (float)((const int32_t*)pcm)[idx] / (bitdepth == 24 ? 256.0f : 65536.0f);
}

/* 48 kHz / 10 ms (one output per 15/4 input samples): which two of the frame's 128 outputs a lane forms.  With outputs (lane, lane + 64) the 32 lanes of
 * a half-wave read from 16 LDS banks (input index ceil(3.75 n) mod 32: two lanes per bank); with this assignment - found by search, tools/rs48_map.py -
 * from 32.  Both outputs of a lane are of the same filter phase (n mod 4). */
__device__ const uint8_t lc3t_rs48_map[128] = {
    12, 28, 36, 48, 52, 84, 100, 116, 25, 41, 57, 61, 85, 93, 109, 125, 18, 26, 30, 54, 90, 98, 106, 122, 3, 19, 27, 51, 55, 67, 83, 111, 20, 44, 60, 72, 76, 88, 96, 108, 13, 33, 49, 53, 69, 73, 81, 101, 6, 10, 34, 38, 46, 58, 62, 114, 15, 35, 39, 43, 59, 91, 99, 119,
    0, 16, 24, 40, 56, 68, 80, 112, 9, 21, 45, 65, 77, 105, 113, 121, 22, 42, 66, 70, 78, 86, 118, 126, 23, 31, 47, 63, 71, 115, 123, 127, 4, 8, 32, 64, 92, 104, 120, 124, 1, 5, 17, 29, 37, 89, 97, 117, 2, 14, 50, 74, 82, 94, 102, 110, 7, 11, 75, 79, 87, 95, 103, 107};

#ifdef LC3_PCM_FMT                 /* the object of the PCM formats beyond 16 / 24 / 32 holds the two resamplers of those formats alone */
#define RESAMPLE_PCM_FMT 1
#else
#define RESAMPLE_PCM_FMT 0
#endif
#include "lc3_enc_resample.inc"    /* lc3_enc_resample_kernel, or lc3_enc_resample_fmt_kernel */

/* ---- 48 kHz / 10 ms (N = 480, one output per 15/4 input samples, 60 taps per output): four outputs per lane --------------------------------------
 * The kernel above reads 2 x 60 words of LDS per output (taps and samples: 61 KB per frame) and is bound by exactly that: 486 LDS-array cycles per
 * frame, 63 % of its wave-cycles stalled on the LDS queue (profiles/r04_diag_pmc.txt: SQ_WAIT_INST_LDS 1 874 of 2 955, SQ_LDS_IDX_ACTIVE 486).
 * Here a lane owns the outputs n = 16 b + 4 k + p, k = 0 ... 3, of one frame: they share the polyphase branch p = n mod 4 - its 60 taps stay in
 * registers for the whole run of frames - and their input windows start 15 samples apart, so the lane reads 108 consecutive samples
 * x[60 b + 4 p ...] ONCE (27 ds_read_b128, 16-byte aligned for every lane) for 240 multiply-adds: 13.8 KB of LDS reads per frame.  32 lanes do a
 * frame, the two halves of a wave two consecutive frames (the second 480 samples further in the same LDS image).  The lane -> (frame, b, p) table makes
 * the sixteen lanes of every ds_read_b128 service group hit sixteen different quad-words mod 16 (tools/rs48_map4.py, tests/test_rs48_map.py).
 * Sums in the reference's order: an output's 60 products are added one by one from tap 0 (R/resamp12k8.c:48-57). */
__device__ const uint8_t lc3t_rs48_lane4[64] = {
    16, 12, 8, 4, 21, 17, 13, 9, 5, 29, 25, 1, 0, 28, 24, 20, 53, 49, 45, 41, 48, 44, 40, 36, 32, 60, 56, 52, 37, 61, 57, 33,
    26, 22, 18, 14, 31, 27, 23, 19, 15, 11, 7, 3, 10, 30, 6, 2, 63, 59, 55, 51, 58, 54, 50, 46, 42, 62, 38, 34, 47, 43, 39, 35};

struct __attribute__((aligned(16))) Pre48Lds { float xs[60 + 2 * 480]; };      /* [previous frame's last 60 samples | frame t | frame t + 1], scaled */

__device__ __forceinline__ void pre48_put(float* __restrict__ d, const uint4 v, const float sf)
{
    float4 a, b;
    a.x = (float)(int16_t)(v.x & 0xffff) * sf; a.y = (float)(int16_t)(v.x >> 16) * sf; a.z = (float)(int16_t)(v.y & 0xffff) * sf; a.w = (float)(int16_t)(v.y >> 16) * sf;
    b.x = (float)(int16_t)(v.z & 0xffff) * sf; b.y = (float)(int16_t)(v.z >> 16) * sf; b.z = (float)(int16_t)(v.w & 0xffff) * sf; b.w = (float)(int16_t)(v.w >> 16) * sf;
    ((float4*)d)[0] = a; ((float4*)d)[1] = b;
}

#if defined(LC3_PCM_PLACED) || (defined(LC3_ENC_RPIPE) && defined(LC3_PCM_FMT))      /* the placed object holds lc3_enc_resample_plc_kernel alone: a placed call always takes the resampler for every shape; so does a ragged call (the typed resamplers have no ragged forms) */
#elif defined(LC3_PCM_FMT)
/* lc3_enc_resample48_kernel (below) for samples that follow each other in the default or the channel-major layout of the format word fmt: its tap and LDS scheme
 * unchanged, only the load and convert step differs.  A frame is 120 pieces of four samples instead of 60 of eight: a lane loads piece lane and piece lane + 60 of
 * both frames of its pair, keeps them as loaded, and writes each to LDS as one float4 - consecutive lanes, consecutive quad-words.  One text, two kernels:
 *   lc3_enc_resample48f_kernel (the _fmt object): float samples, a piece is 16 bytes of a 16-byte aligned frame;
 *   lc3_enc_resample48w_kernel (the _wire object): the five wire types (lc3_plan.h: LC3D_PCM_S16_BE ... LC3D_PCM_ALAW), a piece is one, two or three whole dwords
 *   by the element size of a dword-aligned frame (12 registers for the four pieces, the float kernel has 16), converted by pcm_wire_x4. */
#ifdef LC3_PCM_WIRE
struct Pre48Raw { unsigned a, b, c; };
typedef Pre48Raw pre48_piece;
typedef unsigned pre48_word;                 /* what the frame pointer counts in */
#define PRE48_FN lc3_enc_resample48w_kernel
#define PRE48_WORDS(elems) ((elems) * nd / 4)            /* elements -> words of the frame pointer */
#define PRE48_ZERO {0, 0, 0}
__device__ __forceinline__ pre48_piece pre48_ld(const unsigned* __restrict__ fr, int nd, int piece)
{
    Pre48Raw r = {0, 0, 0};
    const unsigned* p = fr + piece * nd;
    r.a = p[0]; if (nd > 1) r.b = p[1]; if (nd > 2) r.c = p[2];
    return r;
}
__device__ __forceinline__ void pre48_putx(float* __restrict__ d, int ty, const pre48_piece r, const float sf)
{
    const float4 c = pcm_wire_x4(ty, r.a, r.b, r.c);
    *(float4*)d = make_float4(c.x * sf, c.y * sf, c.z * sf, c.w * sf);
}
#else
typedef float4 pre48_piece;
typedef float pre48_word;
#define PRE48_FN lc3_enc_resample48f_kernel
#define PRE48_WORDS(elems) (elems)
#define PRE48_ZERO make_float4(0, 0, 0, 0)
__device__ __forceinline__ pre48_piece pre48_ld(const float* __restrict__ fr, int, int piece) { return ((const float4*)fr)[piece]; }
__device__ __forceinline__ void pre48_putx(float* __restrict__ d, int, const float4 v, const float sf)
{
    const float4 c = pcm_f32x4(v);
    *(float4*)d = make_float4(c.x * sf, c.y * sf, c.z * sf, c.w * sf);
}
#endif

extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(3, 3)))
PRE48_FN(const lc3d_plan* __restrict__ P, const pre48_word* __restrict__ pcm /* 16-byte (float) or 4-byte (wire) aligned */, int fmt, int channels, int memcap,
         int T, int tb, int nt, int ncs, float* __restrict__ d12 /* [cs][T][128] */, const float* __restrict__ xprev, int xprev_stride)
{
    __shared__ Pre48Lds L;
    const int lane = threadIdx.x;
    const int runs = (nt + PRE_FPW - 1) / PRE_FPW;
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * PRE_FPW, t1 = imin(tb + nt, t0 + PRE_FPW);
    if (cs >= ncs) return;
    const int code = lc3t_rs48_lane4[lane], f = code >> 5, b = (code >> 2) & 7, p = code & 3;
    const float sf = P->rs_scale;
    const int strm = cs / channels, ch = cs - strm * channels;
    float tap[60];
#pragma unroll
    for (int m = 0; m < 60; m++) tap[m] = P->rs_taps[p * 60 + m];
    float* xs = L.xs;
    const int ty = fmt & LC3D_PCM_TYPE_MASK, nd = lc3d_pcm_elem_bytes(ty);         /* (wire) dwords per piece of four samples = bytes per element */
    const size_t e0 = lc3d_pcm_frame(fmt, channels, T, 480, strm, t0, ch);         /* frame t0 of this channel-stream, in elements; the next one is fstep further */
    const pre48_word* fr0 = pcm + PRE48_WORDS(e0);
    const size_t fstep = PRE48_WORDS(lc3d_pcm_fstep(fmt, channels, 480));
    pre48_piece fa0 = PRE48_ZERO, fa1 = fa0, fb0 = fa0, fb1 = fa0;
    if (lane < 60) {
        fa0 = pre48_ld(fr0, nd, lane); fa1 = pre48_ld(fr0, nd, lane + 60);
        if (t0 + 1 < t1) { fb0 = pre48_ld(fr0 + fstep, nd, lane); fb1 = pre48_ld(fr0 + fstep, nd, lane + 60); }
    }
    if (lane < 60) {   /* the 60 samples in front of frame t0: from the PCM of this call, or the stream's MDCT memory for its first frame */
        float v;
#ifdef LC3_PCM_WIRE
        if (t0 > 0) v = pcm_wire(pcm, ty, e0 - lc3d_pcm_fstep(fmt, channels, 480) + 420 + lane);
#else
        if (t0 > 0) v = pcm_f32((fr0 - fstep)[420 + lane]);
#endif
        else v = xprev[(size_t)cs * xprev_stride + (memcap - 60 + lane)];
        xs[lane] = v * sf;
    }
    const float4* xb = (const float4*)(xs + 480 * f + 60 * b + 4 * p);
    float* o = d12 + ((size_t)cs * T + t0 + f) * 128 + 16 * b + p;
    for (int t = t0; t < t1; t += 2) {
        float4 tl = make_float4(0, 0, 0, 0);
        if (t > t0 && lane < 15) tl = ((const float4*)xs)[240 + lane];       /* the last 60 samples of the pair before */
        LSYNC();
        if (t > t0 && lane < 15) ((float4*)xs)[lane] = tl;
        if (lane < 60) {
            pre48_putx(xs + 60 + 4 * lane, ty, fa0, sf); pre48_putx(xs + 300 + 4 * lane, ty, fa1, sf); pre48_putx(xs + 540 + 4 * lane, ty, fb0, sf); pre48_putx(xs + 780 + 4 * lane, ty, fb1, sf);
            const pre48_word* fn = fr0 + (size_t)(t + 2 - t0) * fstep;
            if (t + 2 < t1) { fa0 = pre48_ld(fn, nd, lane); fa1 = pre48_ld(fn, nd, lane + 60); }
            if (t + 3 < t1) { fb0 = pre48_ld(fn + fstep, nd, lane); fb1 = pre48_ld(fn + fstep, nd, lane + 60); }
        }
        LSYNC();
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 27; c++) {
            const float4 q = xb[c];
            const float xv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int u = 4 * c + e;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int m = u - 15 * k;
                    if (m >= 0 && m < 60) acc[k] += xv[e] * tap[m];
                }
            }
        }
        if (f == 0 || t + 1 < t1) {
#pragma unroll
            for (int k = 0; k < 4; k++) o[4 * k] = acc[k];
        }
        o += 256;
    }
}
#else
#ifndef LC3_ENC_RPIPE
extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(3, 3)))
lc3_enc_resample48_kernel(const lc3d_plan* __restrict__ P, const int16_t* __restrict__ pcm /* 16-byte aligned */, int channels, int memcap,
                          int T, int tb, int nt, int ncs, float* __restrict__ d12 /* [cs][T][128] */,
                          const float* __restrict__ xprev /* the MDCT / resampler memory before frame 0 (slot of memcap words per channel-stream) */, int xprev_stride)
{
    __shared__ Pre48Lds L;
    const int lane = threadIdx.x;
    const int runs = (nt + PRE_FPW - 1) / PRE_FPW;
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * PRE_FPW, t1 = imin(tb + nt, t0 + PRE_FPW);
    if (cs >= ncs) return;
    const int code = lc3t_rs48_lane4[lane], f = code >> 5, b = (code >> 2) & 7, p = code & 3;
    const float sf = P->rs_scale;
    const int strm = cs / channels, ch = cs - strm * channels;
    float tap[60];
#pragma unroll
    for (int m = 0; m < 60; m++) tap[m] = P->rs_taps[p * 60 + m];
    float* xs = L.xs;
    const int16_t* fr0 = pcm + (((size_t)strm * T + t0) * channels + ch) * 480;             /* frame t0 of this channel-stream; the next one is 480 x channels further */
    const size_t fstep = (size_t)channels * 480;
    uint4 nva = make_uint4(0, 0, 0, 0), nvb = nva;
    if (lane < 60) { nva = ((const uint4*)fr0)[lane]; if (t0 + 1 < t1) nvb = ((const uint4*)(fr0 + fstep))[lane]; }
    if (lane < 60) {   /* the 60 samples in front of frame t0: from the PCM of this call, or the stream's MDCT memory for its first frame */
        float v;
        if (t0 > 0) v = (float)(fr0 - fstep)[420 + lane];
        else v = xprev[(size_t)cs * xprev_stride + (memcap - 60 + lane)];
        xs[lane] = v * sf;
    }
    const float4* xb = (const float4*)(xs + 480 * f + 60 * b + 4 * p);
    float* o = d12 + ((size_t)cs * T + t0 + f) * 128 + 16 * b + p;
    for (int t = t0; t < t1; t += 2) {
        float4 tl = make_float4(0, 0, 0, 0);
        if (t > t0 && lane < 15) tl = ((const float4*)xs)[240 + lane];       /* the last 60 samples of the pair before */
        LSYNC();
        if (t > t0 && lane < 15) ((float4*)xs)[lane] = tl;
        if (lane < 60) { pre48_put(xs + 60 + 8 * lane, nva, sf); pre48_put(xs + 540 + 8 * lane, nvb, sf); }
        if (lane < 60) {
            const int16_t* fn = fr0 + (size_t)(t + 2 - t0) * fstep;
            if (t + 2 < t1) nva = ((const uint4*)fn)[lane];
            if (t + 3 < t1) nvb = ((const uint4*)(fn + fstep))[lane];
        }
        LSYNC();
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 27; c++) {
            const float4 q = xb[c];
            const float xv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int u = 4 * c + e;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int m = u - 15 * k;
                    if (m >= 0 && m < 60) acc[k] += xv[e] * tap[m];
                }
            }
        }
        if (f == 0 || t + 1 < t1) {
#pragma unroll
            for (int k = 0; k < 4; k++) o[4 * k] = acc[k];
        }
        o += 256;
    }
}

/* ---- 96 kHz (one output per 15/2 input samples, 120 taps per output; N = 960 / 480 / 240): four outputs per lane ------------------------------------
 * The same idea as lc3_enc_resample48_kernel for the high-resolution rates, where the two-outputs-per-lane kernel reads 2 x 120 words of LDS per output
 * (c4: 5 623 of the call's 18 300 wave-cycles per frame, c96: 8 070).  A lane owns the outputs n = 8 b + 2 k + p, k = 0 ... 3, of one frame: they share the
 * polyphase branch p = n mod 2 - its 120 taps stay in registers - and their input windows start 15 samples apart at x[60 b + 8 p + 15 k], so the lane reads
 * 168 consecutive samples ONCE (42 ds_read_b128, 16-byte aligned for every lane) for 480 multiply-adds.  A frame is N / 30 lanes (32 / 16 / 8), a wave works on
 * 1 920 samples = 2 / 4 / 8 consecutive frames of its channel-stream at once.  ds_read_b128 is served in four groups of sixteen lanes (MI355X_MICROARCH.md, LDS
 * table; lc3t_b128_slot = group x 16 + place); the quad-word a lane starts at is (N / 4) f + 15 b + 2 p = (N / 4) f - b + 2 p mod 16, so a group that holds one
 * branch p, b = 0 ... BB - 1 and 16 / BB consecutive frames reads sixteen different quad-words mod 16 in every step (N / 4 = 0, 8, 12 mod 16 for the three frame
 * lengths: tests/test_rs48_map.py).  Sums in the reference's order: an output's 120 products are added one by one from tap 0 (R/resamp12k8.c:48-57). */
__device__ const uint8_t lc3t_b128_slot[64] = {
    0, 1, 2, 3, 16, 17, 18, 19, 20, 21, 22, 23, 4, 5, 6, 7, 24, 25, 26, 27, 8, 9, 10, 11, 12, 13, 14, 15, 28, 29, 30, 31,
    32, 33, 34, 35, 48, 49, 50, 51, 52, 53, 54, 55, 36, 37, 38, 39, 56, 57, 58, 59, 40, 41, 42, 43, 44, 45, 46, 47, 60, 61, 62, 63};

struct __attribute__((aligned(16))) Pre96Lds { float xs[120 + 1920 + 8]; };    /* [the 120 samples in front | 1 920 samples = 2 / 4 / 8 frames], scaled */

template <int NF> __device__ __forceinline__ void
resample96_body(Pre96Lds& L, const lc3d_plan* __restrict__ P, const int16_t* __restrict__ pcm /* 16-byte aligned */, int channels, int memcap,
                int T, int tb, int nt, int ncs, float* __restrict__ d12, const float* __restrict__ xprev, int xprev_stride)
{
    constexpr int LPF = NF / 30, FPI = 64 / LPF, BB = LPF / 2, FG = 16 / BB, QPF = NF / 8 /* 16-byte pieces per frame */, FPB = FPI * PRE96_ITERS;
    const int lane = threadIdx.x;
    const int runs = (nt + FPB - 1) / FPB;
    const int cs = blockIdx.x / runs, t0 = tb + (blockIdx.x % runs) * FPB, t1 = imin(tb + nt, t0 + FPB);
    if (cs >= ncs) return;
    const int slot = lc3t_b128_slot[lane], g = slot >> 4, i = slot & 15;
    const int p = g & 1, f = (g >> 1) * FG + i / BB, b = i % BB;
    const float sf = P->rs_scale;
    const int strm = cs / channels, ch = cs - strm * channels;
    float tap[120];
#pragma unroll
    for (int m = 0; m < 120; m++) tap[m] = P->rs_taps[p * 120 + m];
    float* xs = L.xs;
    const size_t fstep = (size_t)channels * NF;
    const int16_t* fr0 = pcm + (((size_t)strm * T + t0) * channels + ch) * NF;               /* frame t0 of this channel-stream; the next one is NF x channels further */
    /* a step's 240 pieces of 16 bytes: piece j = lane + 60 q belongs to frame j / QPF of the step */
    uint4 nv[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        nv[q] = make_uint4(0, 0, 0, 0);
        const int j = lane + 60 * q, fi = j / QPF, w = j - fi * QPF;
        if (lane < 60 && t0 + fi < t1) nv[q] = ((const uint4*)(fr0 + fi * fstep))[w];
    }
    for (int j = lane; j < 120; j += WAVE) {   /* the 120 samples in front of frame t0: from the PCM of this call, or the stream's MDCT memory for its first frame */
        float v;
        if (t0 > 0) v = (float)(fr0 - fstep)[NF - 120 + j];
        else v = xprev[(size_t)cs * xprev_stride + (memcap - 120 + j)];
        xs[j] = v * sf;
    }
    const float4* xb = (const float4*)(xs + NF * f + 60 * b + 8 * p);
    float* o = d12 + ((size_t)cs * T + t0 + f) * 128 + 8 * b + p;
    for (int t = t0; t < t1; t += FPI) {
        float4 tl = make_float4(0, 0, 0, 0);
        if (t > t0 && lane < 30) tl = ((const float4*)xs)[480 + lane];        /* the last 120 samples of the step before */
        LSYNC();
        if (t > t0 && lane < 30) ((float4*)xs)[lane] = tl;
        if (lane < 60) {
#pragma unroll
            for (int q = 0; q < 4; q++) pre48_put(xs + 120 + 8 * (lane + 60 * q), nv[q], sf);
            const int16_t* fn = fr0 + (size_t)(t + FPI - t0) * fstep;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int j = lane + 60 * q, fi = j / QPF, w = j - fi * QPF;
                if (t + FPI + fi < t1) nv[q] = ((const uint4*)(fn + fi * fstep))[w];
            }
        }
        LSYNC();
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 42; c++) {
            const float4 q4 = xb[c];
            const float xv[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int u = 4 * c + e;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int m = u - 15 * k;
                    if (m >= 0 && m < 120) acc[k] += xv[e] * tap[m];
                }
            }
        }
        if (t + f < t1) {
#pragma unroll
            for (int k = 0; k < 4; k++) o[2 * k] = acc[k];
        }
        o += FPI * 128;
    }
}
#define RESAMPLE96_KERNEL(NAME, NF) \
extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(2, 2))) \
NAME(const lc3d_plan* __restrict__ P, const int16_t* __restrict__ pcm, int channels, int memcap, int T, int tb, int nt, int ncs, float* __restrict__ d12, const float* __restrict__ xprev, int xprev_stride) \
{ __shared__ Pre96Lds L; resample96_body<NF>(L, P, pcm, channels, memcap, T, tb, nt, ncs, d12, xprev, xprev_stride); }
RESAMPLE96_KERNEL(lc3_enc_resample96_kernel_n960, 960)
RESAMPLE96_KERNEL(lc3_enc_resample96_kernel_n480, 480)
RESAMPLE96_KERNEL(lc3_enc_resample96_kernel_n240, 240)
#endif /* !LC3_ENC_RPIPE */

/* One channel-stream per lane, all frames of the launch: y = HP50(d), in place.  R/resamp12k8.c:60-74 in the transposed direct form
 * the frame-wise code uses: y1 = b0 x + u11; u11' = (b1 x + u21) - a1 y1; u21' = b2 x - a2 y1. */
#ifndef HP_WHOLE_FRAME
/* A quarter frame (8 x 16 bytes per lane) in flight instead of a whole one: 90 registers instead of 256.  Only ncs / 64 waves exist, each one long dependent
 * chain (ten double-precision instructions per sample, three of them on the recurrence), so a quarter frame - 32 samples, some 2 500 cycles of arithmetic -
 * hides a load as well as a whole frame did; but a wave that wants half a SIMD's registers waits for two one-frame-per-lane waves of another kernel to retire
 * before it can even start, and this kernel sits on the pitch stream's critical path (0.28 ms alone, 0.6 ... 1.5 ms beside the others in round 3's form). */
extern "C" __global__ void __launch_bounds__(WAVE)
ERP_FN(lc3_enc_hp50_kernel)(const lc3d_plan* __restrict__ P, float* __restrict__ state, int state_words, int scal_off, int T, int tb, int nt, int ncs, float* __restrict__ d12 /* [cs][T][128] */ LC3_ERP_OPT)
{
#ifdef HP_PRIO
    __builtin_amdgcn_s_setprio(HP_PRIO);
#endif
    const int cs = blockIdx.x * WAVE + threadIdx.x;
    if (cs >= ncs) return;
#ifdef LC3_ENC_RPIPE                /* ragged: the stream's frames of this launch that are present; none - nothing of the stream is read or written */
    nt = imin(nt, cnt[cs / P->channels] - tb);
    if (nt <= 0) return;
#endif
    const int cpf = P->len12 >> 5;                                         /* chunks of 8 float4 (32 samples) per frame: 4, 2 or 1 */
    const double b0 = lc3t_hp50_b[0], b1 = lc3t_hp50_b[1], b2 = lc3t_hp50_b[2], a1 = lc3t_hp50_a[1], a2 = lc3t_hp50_a[2];
    float* sc = state + (size_t)cs * state_words + scal_off;
    double u11 = (double)sc[F_HP0], u21 = (double)sc[F_HP1];
    float4 cur[8], nxt[8];
    float4* row = (float4*)(d12 + ((size_t)cs * T + tb) * 128);             /* frame t of this stream: row + 32 (t - tb) */
#pragma unroll
    for (int g = 0; g < 8; g++) { cur[g] = row[g]; nxt[g] = cur[g]; }
    for (int t = 0; t < nt; t++) {
        for (int c = 0; c < cpf; c++) {
            float4* p = row + 32 * t + 8 * c;
            const bool more = c + 1 < cpf || t + 1 < nt;
            const float4* q = c + 1 < cpf ? p + 8 : row + 32 * (t + 1);     /* the next chunk: of this frame, or the first of the next */
            if (more) {
#pragma unroll
                for (int g = 0; g < 8; g++) nxt[g] = q[g];
            }
#pragma unroll
            for (int g = 0; g < 8; g++) {
                const float xin[4] = {cur[g].x, cur[g].y, cur[g].z, cur[g].w};
                float yv[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double x = (double)xin[k];
                    const double y1 = b0 * x + u11;
                    const double u1 = (b1 * x + u21) - a1 * y1;
                    const double u2 = b2 * x - a2 * y1;
                    u11 = u1; u21 = u2;
                    yv[k] = (float)y1;
                }
                p[g] = make_float4(yv[0], yv[1], yv[2], yv[3]);
            }
#pragma unroll
            for (int g = 0; g < 8; g++) cur[g] = nxt[g];
        }
        u11 = (double)(float)u11; u21 = (double)(float)u21;            /* the state is a float between frames */
    }
    sc[F_HP0] = (float)u11; sc[F_HP1] = (float)u21;
}
#else
extern "C" __global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(HP_WAVES, HP_WAVES)))
ERP_FN(lc3_enc_hp50_kernel)(const lc3d_plan* __restrict__ P, float* __restrict__ state, int state_words, int scal_off, int T, int tb, int nt, int ncs, float* __restrict__ d12 /* [cs][T][128] */ LC3_ERP_OPT)
{
#ifdef HP_PRIO
    __builtin_amdgcn_s_setprio(HP_PRIO);
#endif
    const int cs = blockIdx.x * WAVE + threadIdx.x;
    if (cs >= ncs) return;
#ifdef LC3_ENC_RPIPE                /* ragged: the stream's frames of this launch that are present; none - nothing of the stream is read or written */
    nt = imin(nt, cnt[cs / P->channels] - tb);
    if (nt <= 0) return;
#endif
    const int ng = P->len12 >> 2;                                          /* float4 groups per frame: 8, 16 or 32 */
    const double b0 = lc3t_hp50_b[0], b1 = lc3t_hp50_b[1], b2 = lc3t_hp50_b[2], a1 = lc3t_hp50_a[1], a2 = lc3t_hp50_a[2];
    float* sc = state + (size_t)cs * state_words + scal_off;
    double u11 = (double)sc[F_HP0], u21 = (double)sc[F_HP1];
    /* Only ncs / 64 waves exist and each is one long dependent chain, so nothing hides a load but the chain itself: the whole next
     * frame (32 x 16 bytes per lane) is requested before the current one is filtered. */
    float4 cur[32], nxt[32];
    {
        const float4* row = (const float4*)(d12 + ((size_t)cs * T + tb) * 128);
#pragma unroll
        for (int g = 0; g < 32; g++) cur[g] = g < ng ? row[g] : make_float4(0, 0, 0, 0);
    }
    for (int t = tb; t < tb + nt; t++) {
        float4* row = (float4*)(d12 + ((size_t)cs * T + t) * 128);
        if (t + 1 < tb + nt) {
            const float4* rn = (const float4*)(row + 32);
#pragma unroll
            for (int g = 0; g < 32; g++) if (g < ng) nxt[g] = rn[g];
        }
#pragma unroll
        for (int g = 0; g < 32; g++) {
            if (g < ng) {
                const float xin[4] = {cur[g].x, cur[g].y, cur[g].z, cur[g].w};
                float yv[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double x = (double)xin[k];
                    const double y1 = b0 * x + u11;
                    const double u1 = (b1 * x + u21) - a1 * y1;
                    const double u2 = b2 * x - a2 * y1;
                    u11 = u1; u21 = u2;
                    yv[k] = (float)y1;
                }
                row[g] = make_float4(yv[0], yv[1], yv[2], yv[3]);
            }
        }
        u11 = (double)(float)u11; u21 = (double)(float)u21;            /* the state is a float between frames */
#pragma unroll
        for (int g = 0; g < 32; g++) cur[g] = nxt[g];
    }
    sc[F_HP0] = (float)u11; sc[F_HP1] = (float)u21;
}
#endif
#endif /* !LC3_PCM_FMT */
