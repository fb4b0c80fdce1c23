/* lc3_host.c -- host side (plain C) of the MI355X LC3plus encode engine.
 *
 * Exports the reference's encoder ABI (include/lc3.h: lc3_enc_*, same semantics as R/lc3.c:102-309 with
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point) plus the batched extension (include/lc3plus_batch.h).
 * All signal processing happens in the HIP kernels (lc3_kernels.hip) reached through lc3_shim.h; this file only
 * derives configuration (R/setup_enc_lc3.c), builds the init-time tables with the host libm exactly where the
 * reference evaluates them, and moves buffers.  There is no CPU encode path: without a HIP device every encode
 * call fails with LC3_ERROR.  The packet layer of the batched extension (probe, ingest, egress, RTP, RTCP, SRTP, RED, FEC) is
 * lc3_packet.c, which sees of a batch only what lc3_batch_view.h hands it.
 */
#include <limits.h>
#include <math.h>
#include <pthread.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/lc3.h"
#include "../../include/lc3plus_batch.h"
#include "lc3_tables.h"
#include "lc3_shim.h"
#include "lc3_probe_shim.h"
#include "lc3_batch_view.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif
#define MAX_CH 2                    /* R/defines.h:121 */
#define IMIN(a, b) ((a) < (b) ? (a) : (b))
#define IMAX(a, b) ((a) > (b) ? (a) : (b))

/* ------------------------------------------------------------------------------------------------ */
/* configuration shared by the single-stream and the batch API                                       */
/* ------------------------------------------------------------------------------------------------ */
typedef struct {
    int fs, fs_in, fs_idx, channels, dms, hrmode;
    float frame_ms;
    int N, ylen, la, nbands, bw_bits, tilt;
    int att_nblocks, att_hang; float att_damping, sns_damping;
    const lc3t_cfg_t* tab;          /* NULL when the frame size has no window/band table */
} geom_t;

static int samplerate_ok(int sr)
{
    switch (sr) { case 8000: case 16000: case 24000: case 32000: case 44100: case 48000: case 96000: return 1; default: return 0; }
}

static void geom_init(geom_t* g, int samplerate, int channels)            /* R/setup_enc_lc3.c:31-70 */
{
    static const int tilts[6] = {14, 18, 22, 26, 30, 34};
    memset(g, 0, sizeof *g);
    g->fs = samplerate == 44100 ? 48000 : samplerate; g->fs_in = samplerate;
    g->fs_idx = g->fs / 10000; if (g->fs_idx > 4) g->fs_idx = 5;
    g->channels = channels; g->dms = 100; g->frame_ms = 10;
    g->tilt = tilts[g->fs_idx];
}

static void geom_update_ex(geom_t* g, int decoder)
{
    if (decoder && g->fs_idx == 5) g->hrmode = 1;                        /* the decoder forces hrmode first: R/setup_dec_lc3.c:76-80 */
    g->N = g->fs / 100;
    if (g->hrmode == 1) { g->ylen = g->N; g->sns_damping = 0.6; }
    else { g->ylen = IMIN(400, g->N); g->sns_damping = 0.85; }
    if (g->fs_idx == 5) g->hrmode = 1;                                    /* reference order kept */
    g->bw_bits = g->hrmode ? 0 : lc3t_bw_bits[g->fs_idx];
    if (g->dms == 100) { g->att_nblocks = 4; g->att_damping = 0.5; g->att_hang = 2; }
    if (g->dms == 25) { g->N >>= 2; g->ylen /= 4; }
    if (g->dms == 50) { g->N >>= 1; g->ylen /= 2; }
    g->tab = NULL; g->nbands = 64; g->la = 0;
    for (int i = 0; i < LC3T_NCFG; i++)
        if (lc3t_cfg[i].valid && lc3t_cfg[i].fs_idx == g->fs_idx && lc3t_cfg[i].dms == g->dms && lc3t_cfg[i].hr == g->hrmode) g->tab = &lc3t_cfg[i];
    if (g->tab) { g->nbands = g->tab->nbands; g->la = g->tab->la_zeros; }
}
static void geom_update(geom_t* g) { geom_update_ex(g, 0); }              /* R/setup_enc_lc3.c:73-193 */

/* The geometry of a call that takes (samplerate, channels, frame_ms, hrmode): a check part, which returns the first error, and a fill part.  Every batch create
 * and every plan hook is these two; a hook that takes one channel passes 1, and the one that checks less (dec_hook_table) calls geom_check_io alone. */
static LC3_Error geom_check_io(int samplerate, int channels)
{
    if (!samplerate_ok(samplerate)) return LC3_SAMPLERATE_ERROR;
    if (channels < 1 || channels > MAX_CH) return LC3_CHANNELS_ERROR;
    return LC3_OK;
}
static LC3_Error geom_check(int samplerate, int channels, float frame_ms, int hrmode, int decoder)
{
    const LC3_Error e = geom_check_io(samplerate, channels);
    if (e) return e;
    { int d = (int)ceil(frame_ms * 10); if (d != 25 && d != 50 && d != 100) return LC3_FRAMEMS_ERROR; }
    if (decoder) {                                                        /* R/lc3.c:350-351: below 44.1 kHz no hrmode, at 96 kHz nothing else */
        if (samplerate < 44100 && hrmode != 0) return LC3_SAMPLERATE_ERROR;
        if (samplerate == 96000 && hrmode == 0) return LC3_HRMODE_ERROR;
    } else if (samplerate < 48000 && hrmode != 0) return LC3_SAMPLERATE_ERROR;
    return LC3_OK;
}
static void geom_fill(geom_t* g, int samplerate, int channels, float frame_ms, int hrmode, int decoder)
{
    geom_init(g, samplerate, channels);
    g->dms = (int)(frame_ms * 10); g->frame_ms = frame_ms; g->hrmode = hrmode > 0;
    geom_update_ex(g, decoder);
}

/* the kernels are built for frame lengths up to LC3D_MAX_N = 960 whose N/2-point DFT has a restated kernel (480 = 15x32, 240 = 15x16,
 * 60 = 4x15, and the prime-factor lengths 10 ... 160) and an MDCT overlap memory of at most 600 samples: every operating point of
 * the reference.  N > 480 or a memory > 300 run in the large-layout kernel (lc3_kernels.hip) */
static int fft_supported(int len);
static int geom_supported(const geom_t* g) { return g->tab && g->N <= LC3D_MAX_N && fft_supported(g->N / 2) && g->N - g->la <= LC3D_MEMCAP_BIG; }

/* R/setup_enc_lc3.c:196-230: the bitrate limits of the geometry (all channels).  Returns an LC3_Error. */
static LC3_Error bitrate_limits(const geom_t* g, int* lo, int* hi)
{
    int minBR = 0, maxBR = 0;
    if (g->hrmode) {
        switch (g->dms) {
        case 25: maxBR = 672000; minBR = g->fs == 48000 ? 172800 : g->fs == 96000 ? 198400 : -1; break;
        case 50: maxBR = 600000; minBR = g->fs == 48000 ? 148800 : g->fs == 96000 ? 174400 : -1; break;
        case 100: maxBR = 500000; minBR = g->fs == 48000 ? 124800 : g->fs == 96000 ? 149600 : -1; break;
        default: return LC3_HRMODE_ERROR;
        }
        if (minBR < 0) return LC3_HRMODE_ERROR;
    } else {
        minBR = 20 * 8 * (1000 / g->frame_ms) * (g->fs_in == 44100 ? 441. / 480 : 1);
        maxBR = 400 * 8 * (1000 / g->frame_ms) * (g->fs_in == 44100 ? 441. / 480 : 1);
    }
    minBR *= g->channels; maxBR *= g->channels;
    *lo = minBR; *hi = maxBR;
    return LC3_OK;
}
/* R/setup_enc_lc3.c:231-375 for one channel of nbytes bytes: everything a bitrate sets is a function of the channel's byte count and the geometry */
static void derive_chan(const geom_t* g, int nbytes, lc3d_chan* s)
{
    s->nbytes = nbytes;
    s->total_bits = s->nbytes << 3;
    s->target_bits_init = s->total_bits - 38 - 8 - 3 - g->bw_bits - (int)ceil(log2f(g->N / 2)) - 2 - 1;
    if (s->total_bits > 1280) s->target_bits_init -= 1;
    if (s->total_bits > 2560) s->target_bits_init -= 1;
    if (g->hrmode) s->target_bits_init -= 1;
    s->lpc_weighting = s->total_bits < 480;
    if (g->frame_ms == 5) s->lpc_weighting = s->total_bits < 240;
    if (g->frame_ms == 2.5) s->lpc_weighting = s->total_bits < 120;
    s->gg_off = -(IMIN(115, s->total_bits / (10 * (g->fs_idx + 1))) + 105 + 5 * (g->fs_idx + 1));
    if (g->frame_ms == 10 && ((g->fs_in >= 44100 && s->nbytes >= 100) || (g->fs_in == 32000 && s->nbytes >= 81)) &&
        s->nbytes < 340 && g->hrmode == 0) s->attack_handling = 1;
    else { s->attack_handling = 0; s->reset_attack = 1; }
    int bitsTmp = s->total_bits;
    if (g->frame_ms == 2.5) bitsTmp = bitsTmp * 4.0 * (1.0 - 0.4);
    if (g->frame_ms == 5) bitsTmp = bitsTmp * 2 - 160;
    s->ltpf_enable = bitsTmp < 640 + (g->fs_idx - 1) * 80;
    if (g->hrmode) s->ltpf_enable = 0;
    if (g->hrmode && g->fs_idx >= 4) {
        int real_rate = s->nbytes * 8000 / g->frame_ms;
        s->reg_bits = real_rate / 12500;
        if (g->fs_idx == 5) { if (g->frame_ms == 10) s->reg_bits += 2; if (g->frame_ms == 2.5) s->reg_bits -= 6; }
        else { if (g->frame_ms == 2.5) s->reg_bits -= 6; if (g->frame_ms == 10) s->reg_bits += 5; }
    } else s->reg_bits = -1;
}
/* R/setup_enc_lc3.c:196-375: bitrate -> per-channel budgets.  Returns an LC3_Error. */
static LC3_Error derive_bitrate(const geom_t* g, int bitrate, lc3d_chan* ch /* [channels] */)
{
    int minBR = 0, maxBR = 0;
    LC3_Error e = bitrate_limits(g, &minBR, &maxBR);
    if (e) return e;
    if (bitrate < minBR || bitrate > maxBR) return LC3_BITRATE_ERROR;
    const int totalBytes = bitrate * g->N / (8 * g->fs_in);
    int off = 0;
    for (int c = 0; c < g->channels; c++) {
        derive_chan(g, totalBytes / g->channels + (c < (totalBytes % g->channels)), &ch[c]);
        ch[c].out_off = off; off += ch[c].nbytes;
        ch[c].bitrate = bitrate;
    }
    return LC3_OK;
}

/* per-frame bitrates: the configuration of every channel byte count 0 .. max, from derive_chan (entry 0 zeroed; out_off and the bandwidth words are
 * not used from it: the kernel takes the channel's offset from the stream-frame size and the bandwidth from the stream) */
/* the largest channel frame of the geometry, encoder and decoder alike (R/defines.h MAX_NBYTES; in hrmode per frame length, R/setup_dec_lc3.c:203-299) */
static int geom_max_chan_bytes(const geom_t* g) { return g->hrmode ? (g->dms == 25 ? 210 : g->dms == 50 ? 375 : 625) : 400; }
static lc3d_chan* enc_build_table(const geom_t* g, int* n)
{
    *n = geom_max_chan_bytes(g) + 1;
    lc3d_chan* tab = (lc3d_chan*)calloc((size_t)*n, sizeof(lc3d_chan));
    if (!tab) return NULL;
    for (int k = 1; k < *n; k++) derive_chan(g, k, &tab[k]);
    return tab;
}
/* The per-frame bitrate rule of lc3plus_enc_batch_encode_bitrates: every rate is checked with the limits of derive_bitrate before anything is written, and
 * gives the stream-frame's byte count as derive_bitrate computes it.  Out: fsz [n] (n = stream-frames), *max_bytes the largest. */
static LC3_Error enc_plan_bitrates(const geom_t* g, const int* bitrates, size_t n, uint16_t* fsz, int* max_bytes)
{
    int lo = 0, hi = 0, mx = 0;
    LC3_Error e = bitrate_limits(g, &lo, &hi);
    if (e) return e;
    for (size_t i = 0; i < n; i++) {
        const int tb = lc3d_enc_rate_bytes(bitrates[i], lo, hi, g->N, g->fs_in, g->channels, geom_max_chan_bytes(g), INT_MAX);   /* (inside the table always, by the limits) */
        if (tb < 0) return LC3_BITRATE_ERROR;
        fsz[i] = (uint16_t)tb;
        if (tb > mx) mx = tb;
    }
    *max_bytes = mx;
    return LC3_OK;
}

/* ---- prime-factor index plan for the 120-point DFT (index logic of R/fft/fft_generic.h:634-699).
 * The recursion is run on slot labels instead of samples: every leaf DFT records where its inputs live in the
 * previous stage's output buffer; its outputs get consecutive slots.  The last stage's scatter is folded in. ---- */
static int pfa_inverse(int a, int b)
{
    int b0 = b, x0 = 0, x1 = 1;
    if (b == 1) return 1;
    while (a > 1) { int q = a / b, t = b; b = a % b; a = t; t = x0; x0 = x1 - q * x0; x1 = t; }
    if (x1 < 0) x1 += b0;
    return x1;
}
typedef struct { uint8_t* src[3]; int count[3]; int leaf[3]; } pfa_rec;
static void pfa_leaf(int* x, int n, pfa_rec* r)
{
    int st = n == r->leaf[0] ? 0 : n == r->leaf[1] ? 1 : 2;
    for (int j = 0; j < n; j++) { r->src[st][r->count[st]] = (uint8_t)x[j]; x[j] = r->count[st]; r->count[st]++; }
}
static void pfa_label(int* x, int length, int* scratch, int nfac, const int* fac, pfa_rec* r)
{
    if (nfac <= 1) { pfa_leaf(x, length, r); return; }
    int* tmp = scratch;
    const int n2 = fac[0], n1 = length / n2, incr = n1 * pfa_inverse(n1, n2);
    int idx = 0, cnt = 0;
    for (int i = 0; i < n1; i++) {
        for (int ii = 0; ii < n2 - 1; ii++) { tmp[cnt++] = x[idx]; idx += incr; if (idx > length) idx -= length; }
        tmp[cnt++] = x[idx]; idx++;
    }
    for (cnt = 0; cnt < length; cnt += n2) pfa_leaf(tmp + cnt, n2, r);
    for (cnt = 0; cnt < n1; cnt++) for (int i = 0; i < n2; i++) x[cnt + i * n1] = tmp[cnt * n2 + i];
    for (cnt = 0; cnt < length; cnt += n1) pfa_label(x + cnt, n1, tmp, nfac - 1, fac + 1, r);
    cnt = 0;
    for (int i = 0; i < n2; i++) {
        idx = i * n1;
        for (int ii = 0; ii < n1; ii++) { tmp[idx] = x[cnt++]; idx += n2; if (idx > length) idx -= length; }
    }
    memcpy(x, tmp, sizeof(int) * length);
}
/* factors: the prime powers of the length in increasing prime order (R/fft/fft_generic.h:89-145 factorize) */
static int pfa_plan(lc3d_plan* p, int len)
{
    static const struct { int len, n, f[3]; } tab[] = {{10, 2, {2, 5, 0}}, {20, 2, {4, 5, 0}}, {30, 3, {2, 3, 5}}, {40, 2, {8, 5, 0}},
                                                        {80, 2, {16, 5, 0}}, {120, 3, {8, 3, 5}}, {160, 2, {32, 5, 0}}};
    if (len == 60) {                                /* 4 x 15 Good-Thomas with the reference's index tables (R/fft/fft_60_128.h:18-23) */
        for (int k = 0; k < 4; k++) for (int l = 0; l < 15; l++) { p->pfa_src[k + 4 * l] = (uint8_t)((45 * k + 16 * l) % 60); p->pfa_dst[k + 4 * l] = (uint8_t)((15 * k + 4 * l) % 60); }
        p->pfa_nst = 0;
        return 1;
    }
    for (unsigned t = 0; t < sizeof tab / sizeof tab[0]; t++) if (tab[t].len == len) {
        int x[LC3D_PFA_STRIDE], scratch[2 * LC3D_PFA_STRIDE];
        pfa_rec r; memset(&r, 0, sizeof r);
        for (int k = 0; k < 3; k++) { r.src[k] = p->pfa_src + LC3D_PFA_STRIDE * k; r.leaf[k] = tab[t].f[k]; p->pfa_rad[k] = tab[t].f[k]; }
        p->pfa_nst = tab[t].n;
        for (int i = 0; i < len; i++) x[i] = i;
        pfa_label(x, len, scratch, tab[t].n, tab[t].f, &r);
        /* x[i] = slot of the last stage holding output bin i  ->  pfa_dst[slot] = i */
        for (int i = 0; i < len; i++) p->pfa_dst[x[i]] = (uint8_t)i;
        return 1;
    }
    return 0;
}
static int fft_supported(int len) { return len == 480 || len == 240 || len == 60 || len == 10 || len == 20 || len == 30 || len == 40 || len == 80 || len == 120 || len == 160; }

/* R/util.h:109 cexpi with the reference's float argument conversion */
static void cexpi_f(float x, float* re, float* im) { *re = cosf(x); *im = sinf(x); }

static void build_plan(const geom_t* g, lc3d_plan* p)
{
    memset(p, 0, sizeof *p);
    p->fs = g->fs; p->fs_idx = g->fs_idx; p->dms = g->dms; p->hrmode = g->hrmode; p->N = g->N; p->ylen = g->ylen; p->la = g->la;
    p->nbands = g->nbands; p->bw_bits = g->bw_bits; p->fft_len = g->N / 2; p->channels = g->channels;
    p->rs_mem_in_len = 2 * 8 * g->fs / 12800;                              /* R/setup_enc_lc3.c:48 */
    p->rs_stride = lc3t_rs_upfac[g->fs_idx]; p->rs_scale = lc3t_rs_scale[g->fs_idx];
    p->len12 = g->dms == 25 ? 32 : g->dms == 50 ? 64 : 128; p->n12 = g->N * 12800 / g->fs;
    {   /* polyphase view of the resampler filter: output n uses phase start = (stride - 15n % stride) % stride, taps lp[239 - start - m*stride] */
        const int st = p->rs_stride, T = 240 / st;
        for (int ph = 0; ph < st; ph++) for (int m = 0; m < T; m++) p->rs_taps[ph * T + m] = lc3t_rs_lp[239 - ph - m * st];
    }
    p->ltpf_mem_len = g->dms == 25 ? 232 + 32 : 232;
    p->att_nblocks = g->att_nblocks; p->att_hang = g->att_hang; p->att_damping = g->att_damping; p->sns_damping = g->sns_damping;
    p->bw_cls = g->dms == 25 ? 0 : g->dms == 50 ? 1 : 2;
    p->win_off = g->tab->win_off; p->band_off = g->tab->band_off; p->tilt = g->tilt; p->frame_ms = g->frame_ms;
    const int len = g->N;
    for (int i = 0; i < len / 2; i++) {                                   /* R/dct4.c:58-61 */
        cexpi_f(-M_PI * (i + 0.25) / len, &p->tw1[2 * i], &p->tw1[2 * i + 1]);
        cexpi_f(-M_PI * i / len, &p->tw2[2 * i], &p->tw2[2 * i + 1]);
    }
    p->dct4_norm = 1.0 / sqrtf(len / 2);                                   /* R/dct4.c:82 */
    for (int i = 0; i < 16; i++) {                                         /* R/dct4.c:43-45 */
        float cr, ci, sr = 2 / sqrtf(2 * 16), si = 0;
        cexpi_f(-M_PI * i / (2 * 16), &cr, &ci);
        p->dct2_tw[2 * i] = cr * sr - ci * si;
        p->dct2_tw[2 * i + 1] = ci * sr + cr * si;
    }
    for (int i = 0; i < 16; i++) for (int j = 0; j < 16; j++)              /* R/sns_quantize_scf.c:30 */
        p->idct_cos[i * 16 + j] = cos(M_PI / (2.0 * (float)16) * (2.0 * ((float)i + 1.0) - 1.0) * ((float)j));
    p->c_idct_n1 = sqrtf(2.0 / (float)16); p->c_idct_n2 = 1.0 / (sqrtf(2.0));
    for (int i = 0; i < 64; i++)                                           /* R/sns_compute_scf.c:91 */
        p->sns_preemph[i] = powf(10.0, (float)i * (float)g->tilt / ((float)64 - 1.0) / 10.0);
    for (int k = -256; k < 256; k++) {
        float ind = (float)k;                                              /* R/estimate_global_gain.c:136: (ind + off) is a float holding k */
        p->gain_est[k + 256] = powf(10.0, (ind / 28.0));
        p->gain_adj[k + 256] = powf(10, (float)(k) / 28);                  /* R/adjust_global_gain.c:47 */
    }
    p->c_1em5_a = powf(10.0, -5.0); p->c_1em5_b = powf(10, -5); p->c_1em4 = powf(10.0, -40.0 / 10.0);
    p->c_2m32 = powf(2.0, -32.0); p->c_2m31 = powf(2, -31); p->c_2m24 = powf(2, -24); p->c_2p15 = powf(2, 15); p->c_2p100 = powf(2, 100);
    p->c_sqrt2 = sqrtf(2);
    {   /* float thresholds equivalent to the reference's double comparisons against float operands */
        const double t7 = (7.0) * (28.0 / 20.0), t50 = (50.0) * (28.0 / 20.0);
        float f = (float)t7; if ((double)f < t7) f = nextafterf(f, INFINITY); p->c_thr7_up = f;
        f = (float)t50; if ((double)f > t50) f = nextafterf(f, -INFINITY); p->c_thr50_dn = f;
    }
    for (int t = 0; t < 1024; t++) {
        unsigned w = 0, e[4];
        for (int j = 0; j < 4; j++) { const unsigned pk = lc3t_ac_ctx_lut[t + 1024 * j]; w |= pk << (8 * j); e[j] = lc3t_ac_bits[pk * 17 + 16]; }
        p->q_lut4[t] = w;
        p->q_esc[t][0] = (uint16_t)e[0]; p->q_esc[t][1] = (uint16_t)(e[0] + e[1]); p->q_esc[t][2] = (uint16_t)(e[0] + e[1] + e[2]); p->q_esc[t][3] = (uint16_t)e[3];
    }
    memcpy(p->q_bits, lc3t_ac_bits, sizeof p->q_bits);
    memset(p->band_of_bin, 255, sizeof p->band_of_bin);
    const uint16_t* be = &lc3t_band_pool[g->tab->band_off];
    for (int b = 0; b < g->nbands; b++) for (int j = be[b]; j < be[b + 1] && j < LC3D_MAX_N; j++) p->band_of_bin[j] = (uint8_t)b;
    if (g->N / 2 != 240 && g->N / 2 != 480) pfa_plan(p, g->N / 2);
}

static void init_state(float* st, int memcap)                             /* zeroed EncSetup + olpa_mem_pitch = 17 (R/setup_enc_lc3.c:178) */
{
    memset(st, 0, sizeof(float) * LC3D_STATE_WORDS(memcap));
    ((int*)st)[LC3D_S_OLPA_PITCH_WORD(memcap)] = 17;
}

/* the decoder's counterpart: zeros; ltpf_mem_beta_idx = -1, cum_alpha = 1, PLC seed 24607 (R/setup_dec_lc3.c:170-183) */
static void dec_init_state(float* st)
{
    memset(st, 0, sizeof(float) * DST_WORDS);
    int* sc = (int*)(st + DST_SCAL);
    sc[DS_BETA_IDX] = -1; ((float*)sc)[DS_CUM_ALPHA] = 1.0f; sc[DS_PLC_SEED] = 24607;
}

/* ---- stream lifecycle (lc3plus_{enc,dec}_batch_{reset,export,import}_streams) ---- */
enum { SS_ENC = 'E', SS_DEC = 'D' };
/* words of one channel-stream's state row: LC3D_STATE_WORDS of the encoder's kernel layout, DST_WORDS for the decoder */
static int stream_row_words(int codec, const geom_t* g)
{
    return codec == SS_DEC ? DST_WORDS : LC3D_STATE_WORDS(LC3D_LAYOUT_BIG(g->N, g->la) ? LC3D_MEMCAP_BIG : LC3D_MEMCAP_STD);
}
/* The header of a stream's blob: "L3S" and the codec, the input sample rate, frame length (ms x 10) | hrmode << 8 | channels << 16, and the row length in
 * words.  Two batches whose blobs carry the same header have the same state layout. */
static void stream_header(int codec, const geom_t* g, uint32_t h[4])
{
    h[0] = 'L' | '3' << 8 | 'S' << 16 | (uint32_t)codec << 24;
    h[1] = (uint32_t)g->fs_in;
    h[2] = (uint32_t)g->dms | (uint32_t)g->hrmode << 8 | (uint32_t)g->channels << 16;
    h[3] = (uint32_t)stream_row_words(codec, g);
}
/* The blob-header rule of an import: a blob is accepted where its first LC3D_SS_HEADER bytes equal the batch's header (the kernel applies the same rule to
 * device blobs) */
static int stream_header_ok(const uint32_t want[4], const void* blob) { return memcmp(want, blob, LC3D_SS_HEADER) == 0; }
static size_t stream_blob_bytes(int codec, const geom_t* g) { return LC3D_SS_HEADER + sizeof(float) * (size_t)g->channels * stream_row_words(codec, g); }
/* The index-list rule of the lifecycle calls: a list, n >= 1, every index in [0, n_streams) and none twice.  Returns an LC3_Error. */
static LC3_Error stream_list_check(int n_streams, const int* streams, int n)
{
    if (!streams) return LC3_NULL_ERROR;
    if (n <= 0 || n_streams <= 0) return LC3_ERROR;
    uint8_t* seen = (uint8_t*)calloc(((size_t)n_streams + 7) / 8, 1);
    if (!seen) return LC3_ERROR;
    LC3_Error e = LC3_OK;
    for (int i = 0; i < n && !e; i++) {
        const int s = streams[i];
        if (s < 0 || s >= n_streams || (seen[s >> 3] >> (s & 7) & 1)) e = LC3_ERROR;
        else seen[s >> 3] |= (uint8_t)(1 << (s & 7));
    }
    free(seen);
    return e;
}
/* the argument checks every export / import shares, before any work */
static LC3_Error stream_blob_check(int n_streams, const int* streams, int n, const void* blob, int blob_on_device)
{
    if (!blob) return LC3_NULL_ERROR;
    LC3_Error e = stream_list_check(n_streams, streams, n);
    if (e) return e;
    return blob_on_device && ((uintptr_t)blob & 15) ? LC3_ERROR : LC3_OK;
}
/* host blobs: every header checked before anything is queued */
static LC3_Error stream_import_host_check(int codec, const geom_t* g, const void* blob, int n)
{
    uint32_t h[4];
    stream_header(codec, g, h);
    const size_t sz = stream_blob_bytes(codec, g);
    for (int i = 0; i < n; i++) if (!stream_header_ok(h, (const uint8_t*)blob + (size_t)i * sz)) return LC3_ERROR;
    return LC3_OK;
}
/* Export and import of both batch kinds: the checks, the batch's header, the device call of the kind (dev: the batch's context).  Reset is per kind: the two
 * configurations differ. */
static int stream_state_call(int codec, void* dev, int mode, const int* streams, int n, void* blob, int blob_on_device, const uint32_t* h, uint8_t* status,
                             void* hip_stream, int sync)
{
    return codec == SS_DEC ? lc3hip_dec_stream_state(dev, mode, streams, n, NULL, blob, blob_on_device, h, status, hip_stream, sync)
                           : lc3hip_stream_state(dev, mode, streams, n, NULL, blob, blob_on_device, h, status, hip_stream, sync);
}
static LC3_Error streams_export(int codec, const geom_t* g, int n_streams, void* dev, const int* streams, int n, void* blob, int blob_on_device, void* hip_stream,
                                int sync)
{
    LC3_Error e = stream_blob_check(n_streams, streams, n, blob, blob_on_device);
    if (e) return e;
    uint32_t h[4];
    stream_header(codec, g, h);
    return stream_state_call(codec, dev, LC3D_SS_EXPORT, streams, n, blob, blob_on_device, h, NULL, hip_stream, sync) ? LC3_ERROR : LC3_OK;
}
static LC3_Error streams_import(int codec, const geom_t* g, int n_streams, void* dev, const int* streams, int n, const void* blob, int blob_on_device,
                                uint8_t* status, void* hip_stream, int sync)
{
    LC3_Error e = stream_blob_check(n_streams, streams, n, blob, blob_on_device);
    if (!e && !blob_on_device) e = stream_import_host_check(codec, g, blob, n);
    if (e) return e;
    uint32_t h[4];
    stream_header(codec, g, h);
    if (stream_state_call(codec, dev, LC3D_SS_IMPORT, streams, n, (void*)blob, blob_on_device, h, status, hip_stream, sync)) return LC3_ERROR;
    if (status && !blob_on_device) memset(status, 0, (size_t)n);
    return LC3_OK;
}

/* ------------------------------------------------------------------------------------------------ */
/* batch object                                                                                      */
/* ------------------------------------------------------------------------------------------------ */
struct lc3plus_batch {
    geom_t g; int n_streams; int stride;
    lc3d_chan* chans;               /* [n_streams * channels] host mirror */
    int* bitrates;
    void* dev;
    uint16_t* fsz; size_t fsz_cap;  /* per-frame bitrates: stream-frame sizes of enc_plan_bitrates, grown as needed */
    uint16_t* bwf; size_t bwf_cap;  /* per-frame bandwidths: the values in force of enc_plan_bandwidths, grown as needed */
    int chans_stale;                /* a call with rates or bandwidths in device memory has changed the configuration on the device: enc_refresh before reading chans */
    int stride_bound;               /* while chans is stale: the out_stride an encode() needs (stride() before those calls, raised to the out_stride of each with rates) */
    int bw_unsafe;                  /* set_bandwidth has installed a value with a cut-off line below 1 since the last read-back */
    int dry;                        /* DRY_*: the call checks its arguments as always and returns before it touches the device (sharded batches) */
    int placed;                     /* lc3plus_enc_batch_set_pcm_placement is on: the calls below refuse host PCM, traces and the channel-major layout */
    int ragged;                     /* lc3plus_enc_batch_set_frame_counts is on: only encode_rates_device and encode_packed encode, the others refuse */
    /* a ragged call has left the copy stale: a stream that was absent from it may still hold a one-shot attack-detector reset in its device configuration
     * (lc3_enc_rates_tail_kernel_rag leaves such a stream alone), which the stale copy does not show.  Until the copy is read back (enc_refresh) or a dense
     * call with words has run (its tail kernel clears every stream's), a call treats resets as pending: the fixed-rate calls read the copy back before they
     * launch, so that they clear and upload as ever instead of leaving the word for their next launch to act on again. */
    int resets_unknown;
};
/* Grows a host scratch array of a batch (fsz, bwf; the decoder's eff, lost) to n >= 1 elements of `size` bytes; what it held is not kept.  Returns the array,
 * or NULL where there is no memory: the old array is gone then and the capacity 0, and the call that asked returns LC3_ERROR. */
static void* scratch_grow(void* p, size_t* cap, size_t n, size_t size)
{
    if (*cap >= n) return p;
    free(p); *cap = 0;
    p = malloc(n * size);
    if (p) *cap = n;
    return p;
}
/* all the packet layer sees of an encoder batch (lc3_batch_view.h) */
lc3host_view lc3host_enc_view(const lc3plus_batch* b) { const lc3host_view v = {b->dev, 0, b->n_streams, b->g.channels, b->g.ylen}; return v; }

/* A sharded batch checks a call on every shard before any shard runs it: the per-batch call itself, stopped behind its checks.  The checks of a call come in
 * the order bandwidth values, rate values, everything else; DRY_BW and DRY_RATES stop behind the first and the second, so that the shards can be walked
 * once per step and the first refusal is the one an unsharded batch of all the streams gives. */
enum { DRY_BW = 1, DRY_RATES = 2, DRY_ALL = 3 };
#define DRY_STOP(b, level, res) do { if ((b)->dry && (b)->dry <= (level)) return (res); } while (0)
static void batch_restride(lc3plus_batch* b);
/* whether the host copy holds a bandwidth with a cut-off line below 1 (bw_unsafe is this or, since the last look, 1 where set_bandwidth installed one) */
static int enc_bw_unsafe(const lc3plus_batch* b)
{
    for (int i = 0; i < b->n_streams; i++) if (!lc3d_bw_value_ok(b->chans[(size_t)i * b->g.channels].bandwidth, b->g.dms)) return 1;
    return 0;
}
/* Brings the host copy of the configuration back after calls with rates or bandwidths in device memory: waits for the batch's last call and downloads it, once. */
static LC3_Error enc_refresh(lc3plus_batch* b)
{
    if (!b->chans_stale) return LC3_OK;
    if (lc3hip_download_chans(b->dev, b->chans)) return LC3_ERROR;
    for (int i = 0; i < b->n_streams; i++) b->bitrates[i] = b->chans[(size_t)i * b->g.channels].bitrate;
    b->bw_unsafe = enc_bw_unsafe(b);
    batch_restride(b);
    b->chans_stale = 0; b->resets_unknown = 0;
    return LC3_OK;
}
/* the smallest out_stride encode() accepts: stride(), or while the host's copy is stale the bound those calls have left (no read-back) */
static int enc_stride_bound(const lc3plus_batch* b) { return b->chans_stale ? b->stride_bound : b->stride; }

static LC3_Error batch_upload(lc3plus_batch* b, int first_stream, int count)
{
    const int C = b->g.channels;
    if (lc3hip_upload_chans(b->dev, b->chans + (size_t)first_stream * C, first_stream * C, count * C)) return LC3_ERROR;
    return LC3_OK;
}

static void batch_restride(lc3plus_batch* b)
{
    int s = 0;
    for (int i = 0; i < b->n_streams; i++) { int n = 0; for (int c = 0; c < b->g.channels; c++) n += b->chans[i * b->g.channels + c].nbytes; s = IMAX(s, n); }
    b->stride = s;
}

/* The end of a call that has launched with host arrays or none (batch_encode, batch_encode_bitrates, batch_encode_bandwidths, encode_packed without words):
 * bitrates NULL or the call's [n_streams][n_frames] rates (checked by enc_plan_bitrates), bwf NULL or the bandwidths in force of enc_plan_bandwidths.  The launch
 * has consumed every one-shot attack-detector reset - those pending from set_bitrate and those the call's own rate changes asked for - and leaves each stream
 * configured with its last frame's rate and the bandwidth in force after its last frame.  The host copy follows and goes to the device only where something
 * changed: the bandwidth words alone where no rate and no reset did (bw_only: a following per-frame-bandwidth call may still overlap this one).  A call with
 * arrays does not wait for its kernels (sync = 0), so its copy is queued behind them on the call's stream; the plain call's is the synchronous one.  A stale
 * copy has no resets to consume (the dense device-word calls consume them, a copy left stale by ragged calls was read back before the launch) and nothing of
 * it is uploaded. */
static LC3_Error enc_call_done(lc3plus_batch* b, const int* bitrates, const uint16_t* bwf, int n_frames, void* hip_stream)
{
    if (b->chans_stale) return LC3_OK;
    const int C = b->g.channels;
    int rate_dirty = 0, bw_dirty = 0;
    for (int i = 0; i < b->n_streams; i++) {
        lc3d_chan* ch = b->chans + (size_t)i * C;
        for (int c = 0; c < C; c++) if (ch[c].reset_attack) { ch[c].reset_attack = 0; rate_dirty = 1; }
        if (bitrates && bitrates[(size_t)i * n_frames + n_frames - 1] != b->bitrates[i]) {
            const int br = bitrates[(size_t)i * n_frames + n_frames - 1];
            if (derive_bitrate(&b->g, br, ch) != LC3_OK) return LC3_ERROR;
            for (int c = 0; c < C; c++) ch[c].reset_attack = 0;          /* (the kernel has done it) */
            b->bitrates[i] = br; rate_dirty = 1;
        }
        if (bwf && bwf[(size_t)i * n_frames + n_frames - 1] != ch[0].bandwidth) {
            const int bw = bwf[(size_t)i * n_frames + n_frames - 1];
            for (int c = 0; c < C; c++) { ch[c].bandwidth = bw; ch[c].bw_cut_bin = lc3d_bw_cut_bin(bw, b->g.dms); ch[c].bw_index = lc3d_bw_index(bw); }
            bw_dirty = 1;
        }
    }
    if (!rate_dirty && !bw_dirty) return LC3_OK;
    if (rate_dirty) batch_restride(b);
    if (!bitrates && !bwf) return batch_upload(b, 0, b->n_streams);
    return lc3hip_upload_chans_async(b->dev, b->chans, 0, b->n_streams * C, hip_stream, !rate_dirty) ? LC3_ERROR : LC3_OK;
}

/* The start of a call whose rates or bandwidths are words in device memory (encode_rates_device, encode_packed).  With bandwidths, a value in force with a
 * cut-off line below 1 is refused as encode_bandwidths refuses it (enc_plan_bandwidths): bw_unsafe says there may be one, the host copy - read back if need be -
 * whether there is.  Out: *resets, whether one-shot attack-detector resets are pending for the launch to consume: those of set_bitrate in a copy that is
 * current, and whatever ragged calls may have left behind a stale one (resets_unknown; a copy left stale by dense calls has none). */
static LC3_Error enc_words_begin(lc3plus_batch* b, int with_bandwidths, int* resets)
{
    if (with_bandwidths && b->bw_unsafe) {
        if (enc_refresh(b)) return LC3_ERROR;
        b->bw_unsafe = enc_bw_unsafe(b);
        if (b->bw_unsafe) return LC3_ERROR;
    }
    *resets = b->resets_unknown;
    if (!b->chans_stale) for (int i = 0; i < b->n_streams * b->g.channels; i++) *resets |= b->chans[i].reset_attack != 0;
    return LC3_OK;
}
/* ... and its end: the configuration after the call is on the device only, and the host copy is read back by the next host-side reader or writer.  Until then
 * encode() checks out_stride against stride_bound: stride() before the first such call, raised to `lim`, the largest stream-frame the call could configure,
 * where the call had rates (every stream-frame of it fits lim, and so does each stream's carry). */
static void enc_words_done(lc3plus_batch* b, int with_rates, int lim)
{
    if (!b->chans_stale) b->stride_bound = b->stride;
    if (with_rates && lim > b->stride_bound) b->stride_bound = lim;
    b->chans_stale = 1;
    b->resets_unknown = b->ragged;              /* a dense call's tail kernel has cleared every stream's reset; a ragged one's only those of the streams that ran */
}

/* the geometry of an encoder batch, or the error create gives for it; no device */
static LC3_Error enc_batch_geometry(geom_t* g, int n_streams, int samplerate, int channels, float frame_ms, int hrmode)
{
    if (n_streams <= 0) return LC3_ERROR;
    const LC3_Error e = geom_check(samplerate, channels, frame_ms, hrmode, 0);
    if (e) return e;
    geom_fill(g, samplerate, channels, frame_ms, hrmode, 0);
    if (!geom_supported(g)) {
        fprintf(stderr, "lc3plus_hip: %d Hz / %.1f ms%s is not built into the gfx950 kernels yet\n", samplerate, frame_ms, hrmode ? " hr" : "");
        return LC3_ERROR;
    }
    return LC3_OK;
}

LC3_Error lc3plus_enc_batch_create(lc3plus_batch** out, int n_streams, int samplerate, int channels, float frame_ms, int hrmode,
                                   const int* bitrates, int device)
{
    if (!out || !bitrates) return LC3_NULL_ERROR;
    *out = NULL;
    geom_t g;
    { LC3_Error e = enc_batch_geometry(&g, n_streams, samplerate, channels, frame_ms, hrmode); if (e) return e; }
    lc3plus_batch* b = (lc3plus_batch*)calloc(1, sizeof *b);
    if (!b) return LC3_ERROR;
    b->g = g;
    b->n_streams = n_streams;
    b->chans = (lc3d_chan*)calloc((size_t)n_streams * channels, sizeof(lc3d_chan));
    b->bitrates = (int*)calloc(n_streams, sizeof(int));
    if (!b->chans || !b->bitrates) { free(b->chans); free(b->bitrates); free(b); return LC3_ERROR; }
    for (int i = 0; i < n_streams; i++) {
        LC3_Error e = derive_bitrate(&b->g, bitrates[i], b->chans + (size_t)i * channels);
        if (e) { free(b->chans); free(b->bitrates); free(b); return e; }
        for (int c = 0; c < channels; c++) b->chans[i * channels + c].reset_attack = 0;
        b->bitrates[i] = bitrates[i];
    }
    batch_restride(b);
    lc3d_plan* plan = (lc3d_plan*)malloc(sizeof *plan);
    float st[LC3D_STATE_WORDS_MAX];
    build_plan(&b->g, plan);
    init_state(st, LC3D_LAYOUT_BIG(b->g.N, b->g.la) ? LC3D_MEMCAP_BIG : LC3D_MEMCAP_STD);
    int rc = lc3hip_create(&b->dev, plan, n_streams, device);
    free(plan);
    if (!rc) rc = lc3hip_set_template(b->dev, st);
    if (!rc) rc = batch_upload(b, 0, n_streams) != LC3_OK;
    if (!rc) { int tab_n = 0; lc3d_chan* tab = enc_build_table(&b->g, &tab_n); rc = !tab || lc3hip_upload_enc_table(b->dev, tab, tab_n); free(tab); }
    if (rc) { if (b->dev) lc3hip_destroy(b->dev); free(b->chans); free(b->bitrates); free(b); return LC3_ERROR; }
    *out = b;
    return LC3_OK;
}

LC3_Error lc3plus_enc_batch_destroy(lc3plus_batch* b)
{
    if (!b) return LC3_NULL_ERROR;
    lc3hip_destroy(b->dev);
    free(b->chans); free(b->bitrates); free(b->fsz); free(b->bwf); free(b);
    return LC3_OK;
}

int lc3plus_enc_batch_input_samples(const lc3plus_batch* b) { return b ? b->g.N : 0; }
/* (the host copy is a cache of the device's configuration: refreshing it leaves the batch as it was) */
int lc3plus_enc_batch_stride(const lc3plus_batch* b) { return b && !enc_refresh((lc3plus_batch*)b) ? b->stride : 0; }
int lc3plus_enc_batch_num_bytes(const lc3plus_batch* b, int stream)
{
    if (!b || stream < 0 || stream >= b->n_streams) return 0;
    if (enc_refresh((lc3plus_batch*)b)) return 0;
    int n = 0;
    for (int c = 0; c < b->g.channels; c++) n += b->chans[stream * b->g.channels + c].nbytes;
    return n;
}

LC3_Error lc3plus_enc_batch_set_bitrate(lc3plus_batch* b, int stream, int bitrate)
{
    if (!b) return LC3_NULL_ERROR;
    if (stream < 0 || stream >= b->n_streams) return LC3_ERROR;
    if (bitrate <= 0) return LC3_BITRATE_ERROR;
    if (enc_refresh(b)) return LC3_ERROR;
    lc3d_chan tmp[MAX_CH];
    memcpy(tmp, b->chans + (size_t)stream * b->g.channels, sizeof(lc3d_chan) * b->g.channels);
    /* a one-shot reset that is still pending - no frame of the stream has run since the rate that asked for it (a stream absent from ragged calls) - stays pending:
     * the reference clears the detector at that set_bitrate, whatever rate follows */
    LC3_Error e = derive_bitrate(&b->g, bitrate, tmp);
    if (e) return e;
    memcpy(b->chans + (size_t)stream * b->g.channels, tmp, sizeof(lc3d_chan) * b->g.channels);
    b->bitrates[stream] = bitrate;
    batch_restride(b);
    return batch_upload(b, stream, 1);
}

LC3_Error lc3plus_enc_batch_set_bandwidth(lc3plus_batch* b, int stream, int bandwidth)   /* R/lc3.c:187-208 */
{
    if (!b) return LC3_NULL_ERROR;
    if (stream < 0 || stream >= b->n_streams) return LC3_ERROR;
    if (b->g.hrmode == 1) return LC3_HRMODE_BW_ERROR;
    if (enc_refresh(b)) return LC3_ERROR;
    lc3d_chan* ch = b->chans + (size_t)stream * b->g.channels;
    int eff = b->g.fs_in;
    if (ch[0].bandwidth != bandwidth) {
        if (b->g.fs_in > 40000) eff = 40000;
        if (bandwidth * 2 > eff) return LC3_BW_WARNING;
        for (int c = 0; c < b->g.channels; c++) {
            ch[c].bandwidth = bandwidth;
            ch[c].bw_cut_bin = lc3d_bw_cut_bin(bandwidth, b->g.dms);
            ch[c].bw_index = lc3d_bw_index(bandwidth);
        }
        if (!lc3d_bw_value_ok(bandwidth, b->g.dms)) b->bw_unsafe = 1;
        return batch_upload(b, stream, 1);
    }
    return LC3_OK;
}

/* The PCM format word of every batch call that takes PCM (include/lc3plus_batch.h: LC3PLUS_PCM_*; the arithmetic is lc3_plan.h's, shared with the kernels):
 * 16, 24, 32 or LC3PLUS_PCM_FLOAT32, alone or with one of the two layout bits. */
typedef char pcm_format_words_agree[(LC3PLUS_PCM_FLOAT32 == LC3D_PCM_FLOAT32 && LC3PLUS_PCM_INTERLEAVED == LC3D_PCM_INTERLEAVED &&
                                    LC3PLUS_PCM_CHANNEL_MAJOR == LC3D_PCM_CHANNEL_MAJOR && LC3PLUS_PCM_S16_BE == LC3D_PCM_S16_BE &&
                                    LC3PLUS_PCM_S24_3LE == LC3D_PCM_S24_3LE && LC3PLUS_PCM_S24_3BE == LC3D_PCM_S24_3BE &&
                                    LC3PLUS_PCM_ULAW == LC3D_PCM_ULAW && LC3PLUS_PCM_ALAW == LC3D_PCM_ALAW) ? 1 : -1];
static int pcm_format_plain(int format) { return format == 16 || format == 24 || format == 32; }
/* Host-only hooks: the format check and the address rule without a GPU (tests/test_pcm_format_cpu.py). */
LC3_Error lc3plus_pcm_format_check(int format) { return lc3d_pcm_format_ok(format) ? LC3_OK : LC3_ERROR; }
int64_t lc3plus_pcm_offset(int format, int channels, int n_frames, int samples, int stream, int frame, int channel, int sample)
{
    if (!lc3d_pcm_format_ok(format) || channels <= 0 || n_frames <= 0 || samples <= 0 || stream < 0 || frame < 0 || frame >= n_frames || channel < 0 ||
        channel >= channels || sample < 0 || sample >= samples) return -1;
    return (int64_t)(lc3d_pcm_frame(format, channels, n_frames, samples, stream, frame, channel) + (size_t)sample * lc3d_pcm_stride(format, channels));
}

int lc3plus_pcm_elem_bytes(int format) { return lc3d_pcm_format_ok(format) ? lc3d_pcm_elem_bytes(format) : -1; }
/* Placed PCM (lc3_plan.h: lc3d_pcm_placed_*, the text the _plc kernels compile too).  Host-only hooks: the address rule and the validity rule without a GPU
 * (tests/test_pcm_placed_cpu.py). */
int64_t lc3plus_pcm_placed_offset(int format, int channels, int samples, int64_t frame_offset, int channel, int sample)
{
    if (!lc3d_pcm_format_ok(format) || (format & LC3D_PCM_CHANNEL_MAJOR) || channels <= 0 || samples <= 0 || frame_offset < 0 || channel < 0 || channel >= channels ||
        sample < 0 || sample >= samples) return -1;
    if (frame_offset > INT64_MAX - (int64_t)channels * samples) return -1;
    return (int64_t)(lc3d_pcm_placed_frame(format, channels, samples, (long long)frame_offset, channel) + (size_t)sample * lc3d_pcm_stride(format, channels));
}
LC3_Error lc3plus_plan_placed(int format, int channels, int samples, const int64_t* offsets, int64_t n, int64_t capacity, uint8_t* invalid)
{
    if (n < 0 || capacity < 0 || channels <= 0 || samples <= 0 || !lc3d_pcm_format_ok(format) || (format & LC3D_PCM_CHANNEL_MAJOR)) return LC3_ERROR;
    if (n > 0 && (!offsets || !invalid)) return LC3_NULL_ERROR;
    for (int64_t i = 0; i < n; i++) invalid[i] = (uint8_t)!lc3d_pcm_placed_ok((long long)offsets[i], channels, samples, (long long)capacity);
    return LC3_OK;
}
/* while placement is on: a call with host PCM, a traced call and the channel-major layout are refused before anything else of the call is looked at */
static int placed_refuses(int placed, int pcm_on_device, int format, const void* trace)
{
    return placed && (!pcm_on_device || trace || (format & LC3D_PCM_CHANNEL_MAJOR));
}
LC3_Error lc3plus_enc_batch_set_pcm_placement(lc3plus_batch* b, const int64_t* offsets, int64_t capacity)
{
    if (!b) return LC3_NULL_ERROR;
    if (capacity < 0) return LC3_ERROR;
    if (lc3hip_set_pcm_placement(b->dev, (const long long*)offsets, (long long)capacity)) return LC3_ERROR;
    b->placed = offsets != NULL;
    return LC3_OK;
}
/* records the pointer (the runtime keeps it); from here on the host-pointer, fixed-rate and host-array calls refuse (batch_encode ...) */
LC3_Error lc3plus_enc_batch_set_frame_counts(lc3plus_batch* b, const int32_t* counts)
{
    if (!b) return LC3_NULL_ERROR;
    if (lc3hip_set_frame_counts(b->dev, counts)) return LC3_ERROR;
    b->ragged = counts != NULL;
    return LC3_OK;
}
/* The wire types' conversion rule on the host (lc3_plan.h: the text the kernels compile too), element by element, byte by byte: no alignment needed on the wire side. */
LC3_Error lc3plus_pcm_to_native(int format, const void* src, int64_t n, void* dst)
{
    const int ty = format & LC3D_PCM_TYPE_MASK;
    if (!src || !dst) return LC3_NULL_ERROR;
    if ((format & ~(LC3D_PCM_TYPE_MASK | LC3D_PCM_LAYOUT_MASK)) || !lc3d_pcm_type_wire(ty) || n < 0) return LC3_ERROR;
    const uint8_t* s = (const uint8_t*)src;
    for (int64_t i = 0; i < n; i++) {
        if (ty == LC3D_PCM_ULAW || ty == LC3D_PCM_ALAW) ((int16_t*)dst)[i] = (int16_t)lc3d_g711_expand(s[i], ty == LC3D_PCM_ALAW);
        else if (ty == LC3D_PCM_S16_BE) ((int16_t*)dst)[i] = (int16_t)((s[2 * i] << 8) | s[2 * i + 1]);
        else {
            const int lo = ty == LC3D_PCM_S24_3LE ? 0 : 2;
            ((int32_t*)dst)[i] = (int32_t)(int8_t)s[3 * i + 2 - lo] * 65536 + ((s[3 * i + 1] << 8) | s[3 * i + lo]);
        }
    }
    return LC3_OK;
}
LC3_Error lc3plus_pcm_from_native(int format, const void* src, int64_t n, void* dst)
{
    const int ty = format & LC3D_PCM_TYPE_MASK;
    if (!src || !dst) return LC3_NULL_ERROR;
    if ((format & ~(LC3D_PCM_TYPE_MASK | LC3D_PCM_LAYOUT_MASK)) || !lc3d_pcm_type_wire(ty) || n < 0) return LC3_ERROR;
    uint8_t* d = (uint8_t*)dst;
    for (int64_t i = 0; i < n; i++) {
        if (ty == LC3D_PCM_ULAW || ty == LC3D_PCM_ALAW) d[i] = (uint8_t)lc3d_g711_compress(((const int16_t*)src)[i], ty == LC3D_PCM_ALAW);
        else if (ty == LC3D_PCM_S16_BE) { const uint16_t v = (uint16_t)((const int16_t*)src)[i]; d[2 * i] = (uint8_t)(v >> 8); d[2 * i + 1] = (uint8_t)v; }
        else {
            const uint32_t v = (uint32_t)lc3d_pcm_sat24(((const int32_t*)src)[i]);
            const int lo = ty == LC3D_PCM_S24_3LE ? 0 : 2;
            d[3 * i + lo] = (uint8_t)v; d[3 * i + 1] = (uint8_t)(v >> 8); d[3 * i + 2 - lo] = (uint8_t)(v >> 16);
        }
    }
    return LC3_OK;
}

static LC3_Error batch_encode(lc3plus_batch* b, const void* pcm, int pcm_on_device, int bitdepth, int n_frames, void* out, int out_stride,
                              int out_on_device, void* hip_stream, int sync, void* trace)
{
    if (!b || !pcm || !out) return LC3_NULL_ERROR;
    if (!lc3d_pcm_format_ok(bitdepth)) return LC3_ERROR;
    if (placed_refuses(b->placed, pcm_on_device, bitdepth, trace)) return LC3_ERROR;
    if (b->ragged) return LC3_ERROR;                                 /* per-stream frame counts are read by the calls with flags in device memory alone; nothing is touched here */
    if (trace && !pcm_format_plain(bitdepth)) return LC3_ERROR;      /* the traced calls take the integer formats in the default layout only */
    if (n_frames <= 0 || out_stride < enc_stride_bound(b)) return LC3_ERROR;
    DRY_STOP(b, DRY_ALL, LC3_OK);
    if (b->resets_unknown && enc_refresh(b)) return LC3_ERROR;      /* behind ragged calls: the resets this launch consumes are cleared below, once */
    if (lc3hip_encode(b->dev, pcm, pcm_on_device, bitdepth, n_frames, out, out_stride, out_on_device, hip_stream, sync, trace, NULL, NULL)) return LC3_ERROR;
    return enc_call_done(b, NULL, NULL, n_frames, hip_stream);
}

LC3_Error lc3plus_enc_batch_encode(lc3plus_batch* b, const void* pcm, int pcm_on_device, int bitdepth, int n_frames, void* out,
                                   int out_stride, int out_on_device, void* hip_stream, int sync)
{
    return batch_encode(b, pcm, pcm_on_device, bitdepth, n_frames, out, out_stride, out_on_device, hip_stream, sync, NULL);
}

static LC3_Error batch_encode_bitrates(lc3plus_batch* b, const void* pcm, int pcm_on_device, int bitdepth, const int* bitrates, int n_frames, void* out,
                                       int out_stride, int out_on_device, int* num_bytes, void* hip_stream, int sync, void* trace)
{
    if (!b || !pcm || !out || !bitrates) return LC3_NULL_ERROR;
    if (!lc3d_pcm_format_ok(bitdepth)) return LC3_ERROR;
    if (placed_refuses(b->placed, pcm_on_device, bitdepth, trace)) return LC3_ERROR;
    if (b->ragged) return LC3_ERROR;                                 /* as in batch_encode */
    if (trace && !pcm_format_plain(bitdepth)) return LC3_ERROR;
    if (n_frames <= 0) return LC3_ERROR;
    if (enc_refresh(b)) return LC3_ERROR;
    const size_t n = (size_t)b->n_streams * n_frames;
    b->fsz = (uint16_t*)scratch_grow(b->fsz, &b->fsz_cap, n, sizeof(uint16_t));
    if (!b->fsz) return LC3_ERROR;
    int max_bytes = 0;
    LC3_Error e = enc_plan_bitrates(&b->g, bitrates, n, b->fsz, &max_bytes);
    if (e) return e;
    DRY_STOP(b, DRY_RATES, LC3_OK);
    if (out_stride < max_bytes) return LC3_ERROR;
    DRY_STOP(b, DRY_ALL, LC3_OK);
    if (lc3hip_encode(b->dev, pcm, pcm_on_device, bitdepth, n_frames, out, out_stride, out_on_device, hip_stream, sync, trace, b->fsz, NULL)) return LC3_ERROR;
    if (num_bytes) for (size_t i = 0; i < n; i++) num_bytes[i] = b->fsz[i];
    return enc_call_done(b, bitrates, NULL, n_frames, hip_stream);
}
LC3_Error lc3plus_enc_batch_encode_bitrates(lc3plus_batch* b, const void* pcm, int pcm_on_device, int bitdepth, const int* bitrates, int n_frames, void* out,
                                            int out_stride, int out_on_device, int* num_bytes, void* hip_stream, int sync)
{
    return batch_encode_bitrates(b, pcm, pcm_on_device, bitdepth, bitrates, n_frames, out, out_stride, out_on_device, num_bytes, hip_stream, sync, NULL);
}
/* debug entry point used by tests: encode_bitrates with host pointers and one lc3d_trace per channel-frame */
LC3_Error lc3plus_enc_batch_encode_bitrates_traced(lc3plus_batch* b, const void* pcm, int bitdepth, const int* bitrates, int n_frames, void* out, int out_stride,
                                                   void* traces)
{
    if (!traces) return LC3_NULL_ERROR;
    return batch_encode_bitrates(b, pcm, 0, bitdepth, bitrates, n_frames, out, out_stride, 0, NULL, NULL, 1, traces);
}
/* ---- per-frame bandwidths (lc3plus_enc_batch_encode_bandwidths) ---- */
/* The values a call refuses outright (lc3d_bw_value_ok: lc3d_bw_cut_bin(bw, dms) >= 1, without overflow): a negative bandwidth, and a positive one whose
 * cut-off line is below 1 (the controller would write in front of the spectrum, R/cutoff_bandwidth.c:17-19).  0 switches the controller off.
 * The per-frame rule: frame t of stream s applies lc3_enc_set_bandwidth(bandwidths[s][t]) to the value in force before it (start[s] for frame 0,
 * R/lc3.c:187-208): a new value that 2 * bw > min(fs_in, 40000) refuses keeps the value in force and makes the call's result LC3_BW_WARNING.  Values
 * have been checked with lc3d_bw_value_ok; start values are what set_bandwidth accepted, and one with a cut-off line below 1 that stays in force is refused
 * here too.  Out: in_force [n_streams][n_frames]. */
static LC3_Error enc_plan_bandwidths(const geom_t* g, int n_streams, const int* start, const int* bandwidths, int n_frames, uint16_t* in_force)
{
    const int eff = g->fs_in > 40000 ? 40000 : g->fs_in;
    LC3_Error res = LC3_OK;
    for (int s = 0; s < n_streams; s++) {
        int cur = start[s];
        for (int t = 0; t < n_frames; t++) {
            const int f = lc3d_enc_bw_step(&cur, bandwidths[(size_t)s * n_frames + t], eff / 2, g->dms);     /* 2 * v > eff: eff is even */
            if (f & LC3D_ENC_FL_BW_RANGE) return LC3_ERROR;                                                     /* (checked before) */
            if (f & LC3D_ENC_FL_BW_REFUSED) res = LC3_BW_WARNING;
            if (!lc3d_bw_value_ok(cur, g->dms) || cur > 0xFFFF) return LC3_ERROR;
            in_force[(size_t)s * n_frames + t] = (uint16_t)cur;
        }
    }
    return res;
}
static LC3_Error batch_encode_bandwidths(lc3plus_batch* b, const void* pcm, int pcm_on_device, int bitdepth, const int* bandwidths, const int* bitrates,
                                         int n_frames, void* out, int out_stride, int out_on_device, int* num_bytes, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    if (placed_refuses(b->placed, pcm_on_device, lc3d_pcm_format_ok(bitdepth) ? bitdepth : 0, NULL)) return LC3_ERROR;
    if (b->ragged) return LC3_ERROR;                                 /* as in batch_encode */
    if (b->g.hrmode) return LC3_HRMODE_BW_ERROR;
    if (enc_refresh(b)) return LC3_ERROR;
    const size_t n = (size_t)b->n_streams * (n_frames > 0 ? n_frames : 0);
    if (bandwidths) for (size_t i = 0; i < n; i++) if (!lc3d_bw_value_ok(bandwidths[i], b->g.dms)) return LC3_ERROR;
    DRY_STOP(b, DRY_BW, LC3_OK);
    if (!pcm || !out || !bandwidths) return LC3_NULL_ERROR;
    if (!lc3d_pcm_format_ok(bitdepth)) return LC3_ERROR;
    if (n_frames <= 0) return LC3_ERROR;
    if (bitrates) {
        b->fsz = (uint16_t*)scratch_grow(b->fsz, &b->fsz_cap, n, sizeof(uint16_t));
        if (!b->fsz) return LC3_ERROR;
        int max_bytes = 0;
        LC3_Error e = enc_plan_bitrates(&b->g, bitrates, n, b->fsz, &max_bytes);
        if (e) return e;
        DRY_STOP(b, DRY_RATES, LC3_OK);
        if (out_stride < max_bytes) return LC3_ERROR;
    } else if (out_stride < b->stride) return LC3_ERROR;
    b->bwf = (uint16_t*)scratch_grow(b->bwf, &b->bwf_cap, n, sizeof(uint16_t));
    if (!b->bwf) return LC3_ERROR;
    int start[256];
    LC3_Error res = LC3_OK;
    for (int s0 = 0; s0 < b->n_streams; s0 += 256) {          /* the value in force before the call: the stream's configuration */
        const int m = IMIN(256, b->n_streams - s0);
        for (int i = 0; i < m; i++) start[i] = b->chans[(size_t)(s0 + i) * b->g.channels].bandwidth;
        const LC3_Error e = enc_plan_bandwidths(&b->g, m, start, bandwidths + (size_t)s0 * n_frames, n_frames, b->bwf + (size_t)s0 * n_frames);
        if (e != LC3_OK && e != LC3_BW_WARNING) return e;
        if (e) res = e;
    }
    DRY_STOP(b, DRY_ALL, res);
    if (lc3hip_encode(b->dev, pcm, pcm_on_device, bitdepth, n_frames, out, out_stride, out_on_device, hip_stream, sync, NULL, bitrates ? b->fsz : NULL,
                      b->bwf)) return LC3_ERROR;
    if (num_bytes) for (size_t i = 0; i < n; i++) num_bytes[i] = bitrates ? b->fsz[i] : lc3plus_enc_batch_num_bytes(b, (int)(i / n_frames));
    return enc_call_done(b, bitrates, b->bwf, n_frames, hip_stream) ? LC3_ERROR : res;
}
LC3_Error lc3plus_enc_batch_encode_bandwidths(lc3plus_batch* b, const void* pcm, int pcm_on_device, int bitdepth, const int* bandwidths, const int* bitrates,
                                              int n_frames, void* out, int out_stride, int out_on_device, int* num_bytes, void* hip_stream, int sync)
{
    return batch_encode_bandwidths(b, pcm, pcm_on_device, bitdepth, bandwidths, bitrates, n_frames, out, out_stride, out_on_device, num_bytes, hip_stream, sync);
}
int lc3plus_enc_batch_bandwidth(const lc3plus_batch* b, int stream)
{
    if (!b || stream < 0 || stream >= b->n_streams) return -1;
    if (enc_refresh((lc3plus_batch*)b)) return -1;
    return b->chans[(size_t)stream * b->g.channels].bandwidth;
}
/* the per-frame bandwidth rule for a geometry, without a device: start [n_streams], bandwidths [n_streams * n_frames] -> in_force [n_streams * n_frames].
 * Returns LC3_OK, LC3_BW_WARNING where a value was refused, or the error of the call. */
LC3_Error lc3plus_enc_plan_bandwidths(int samplerate, float frame_ms, int hrmode, int n_streams, const int* start, const int* bandwidths, int n_frames,
                                      int* in_force)
{
    if (!start || !bandwidths || !in_force) return LC3_NULL_ERROR;
    if (n_streams <= 0 || n_frames <= 0) return LC3_ERROR;
    LC3_Error e = geom_check(samplerate, 1, frame_ms, hrmode, 0);
    if (e) return e;
    geom_t g;
    geom_fill(&g, samplerate, 1, frame_ms, hrmode, 0);
    if (g.hrmode) return LC3_HRMODE_BW_ERROR;
    const size_t n = (size_t)n_streams * n_frames;
    for (size_t i = 0; i < n; i++) if (!lc3d_bw_value_ok(bandwidths[i], g.dms)) return LC3_ERROR;
    uint16_t* f = (uint16_t*)malloc(n * sizeof(uint16_t));
    if (!f) return LC3_ERROR;
    e = enc_plan_bandwidths(&g, n_streams, start, bandwidths, n_frames, f);
    if (e == LC3_OK || e == LC3_BW_WARNING) for (size_t i = 0; i < n; i++) in_force[i] = f[i];
    free(f);
    return e;
}

/* test hook: the per-frame bitrate rule for a geometry, without a device.  num_bytes [n_streams * n_frames] out, *max_bytes the largest */
LC3_Error lc3plus_enc_plan_bitrates(int samplerate, int channels, float frame_ms, int hrmode, int n_streams, const int* bitrates, int n_frames,
                                    int* num_bytes, int* max_bytes)
{
    if (!bitrates || !num_bytes || !max_bytes) return LC3_NULL_ERROR;
    if (n_streams <= 0 || n_frames <= 0) return LC3_ERROR;
    LC3_Error e = geom_check(samplerate, channels, frame_ms, hrmode, 0);
    if (e) return e;
    geom_t g;
    geom_fill(&g, samplerate, channels, frame_ms, hrmode, 0);
    const size_t n = (size_t)n_streams * n_frames;
    uint16_t* fsz = (uint16_t*)malloc(n * sizeof(uint16_t));
    if (!fsz) return LC3_ERROR;
    e = enc_plan_bitrates(&g, bitrates, n, fsz, max_bytes);
    if (!e) for (size_t i = 0; i < n; i++) num_bytes[i] = fsz[i];
    free(fsz);
    return e;
}

/* ---- per-frame rates and bandwidths in device memory (lc3plus_enc_batch_encode_rates_device) ---- */
/* the constants of lc3d_enc_frame_step for a geometry; lim: the largest stream-frame the call may write */
static LC3_Error enc_rate_rule(const geom_t* g, int lim, lc3d_rate_rule* r)
{
    LC3_Error e = bitrate_limits(g, &r->lo, &r->hi);
    if (e) return e;
    r->N = g->N; r->fs_in = g->fs_in; r->channels = g->channels; r->max_chan = geom_max_chan_bytes(g); r->lim = lim;
    r->half = (g->fs_in > 40000 ? 40000 : g->fs_in) / 2; r->dms = g->dms;
    return LC3_OK;
}
LC3_Error lc3plus_enc_batch_encode_rates_device(lc3plus_batch* b, const void* pcm, int bitdepth, const int32_t* bitrates, const int32_t* bandwidths,
                                                int n_frames, void* out, int out_stride, int32_t* num_bytes, uint8_t* flags, void* hip_stream, int sync)
{
    if (!b || !pcm || !out || (!bitrates && !bandwidths)) return LC3_NULL_ERROR;
    if (!lc3d_pcm_format_ok(bitdepth)) return LC3_ERROR;
    if (placed_refuses(b->placed, 1, bitdepth, NULL)) return LC3_ERROR;
    if (n_frames <= 0 || out_stride < enc_stride_bound(b)) return LC3_ERROR;
    if (bandwidths && b->g.hrmode) return LC3_HRMODE_BW_ERROR;
    int resets = 0;
    if (enc_words_begin(b, bandwidths != NULL, &resets)) return LC3_ERROR;
    lc3d_rate_rule r;
    if (enc_rate_rule(&b->g, out_stride, &r)) return LC3_ERROR;
    if (lc3hip_encode_rates_device(b->dev, pcm, bitdepth, n_frames, out, out_stride, bitrates, bandwidths, &r, num_bytes, flags, resets, hip_stream, sync))
        return LC3_ERROR;
    enc_words_done(b, bitrates != NULL, out_stride);
    return LC3_OK;
}
/* test hook: the rule of encode_rates_device on host arrays, without a device.  start_rates, start_bw [n_streams]: the stream's configuration before
 * the call; bitrates, bandwidths: NULL or [n_streams][n_frames]; out: num_bytes, bw_in_force, flags [n_streams][n_frames], end_rates [n_streams] */
static LC3_Error enc_plan_rates_host(int samplerate, int channels, float frame_ms, int hrmode, int n_streams, const int* start_rates, const int* start_bw,
                                     const int* bitrates, const int* bandwidths, int n_frames, int out_stride, int* num_bytes, int* bw_in_force,
                                     uint8_t* flags, int* end_rates, const int32_t* counts, int need_words)
{
    if (!start_rates || !start_bw || !num_bytes || !bw_in_force || !flags || !end_rates || (need_words && !bitrates && !bandwidths)) return LC3_NULL_ERROR;
    if (n_streams <= 0 || n_frames <= 0) return LC3_ERROR;
    LC3_Error e = geom_check(samplerate, channels, frame_ms, hrmode, 0);
    if (e) return e;
    geom_t g;
    geom_fill(&g, samplerate, channels, frame_ms, hrmode, 0);
    if (bandwidths && g.hrmode) return LC3_HRMODE_BW_ERROR;
    lc3d_rate_rule r;
    e = enc_rate_rule(&g, out_stride, &r);
    if (e) return e;
    for (int s = 0; s < n_streams; s++) {       /* the start: a configuration the batch can hold, and one the call accepts */
        if (lc3d_enc_rate_bytes(start_rates[s], r.lo, r.hi, r.N, r.fs_in, r.channels, r.max_chan, out_stride) < 0) return LC3_BITRATE_ERROR;
        if (bandwidths && !lc3d_bw_value_ok(start_bw[s], g.dms)) return LC3_ERROR;
    }
    for (int s = 0; s < n_streams; s++) {
        int rate = start_rates[s], bytes = lc3d_enc_rate_bytes(rate, r.lo, r.hi, r.N, r.fs_in, r.channels, r.max_chan, out_stride), bw = start_bw[s];
        const int c = counts ? lc3d_dec_count_clamp(counts[s], n_frames) : n_frames;       /* the frames present; the rest are absent and not looked at */
        for (int t = 0; t < c; t++) {
            const size_t i = (size_t)s * n_frames + t;
            flags[i] = (uint8_t)lc3d_enc_frame_step(&r, bitrates != NULL, bitrates ? bitrates[i] : 0, bandwidths != NULL, bandwidths ? bandwidths[i] : 0,
                                                    &rate, &bytes, &bw);
            num_bytes[i] = bytes; bw_in_force[i] = bw;
        }
        for (int t = c; t < n_frames; t++) { const size_t i = (size_t)s * n_frames + t; flags[i] = LC3D_ENC_FL_ABSENT; num_bytes[i] = 0; bw_in_force[i] = 0; }
        end_rates[s] = rate;
    }
    return LC3_OK;
}
LC3_Error lc3plus_enc_plan_rates_lenient(int samplerate, int channels, float frame_ms, int hrmode, int n_streams, const int* start_rates, const int* start_bw,
                                         const int* bitrates, const int* bandwidths, int n_frames, int out_stride, int* num_bytes, int* bw_in_force,
                                         uint8_t* flags, int* end_rates)
{
    return enc_plan_rates_host(samplerate, channels, frame_ms, hrmode, n_streams, start_rates, start_bw, bitrates, bandwidths, n_frames, out_stride, num_bytes,
                               bw_in_force, flags, end_rates, NULL, 1);
}
/* test hook: the same rule with per-stream frame counts (lc3plus_enc_batch_set_frame_counts): counts NULL or host [n_streams]; bitrates and bandwidths may both
 * be NULL (a ragged encode_packed call with neither: every present frame has the carried size) */
LC3_Error lc3plus_enc_plan_rates_ragged(int samplerate, int channels, float frame_ms, int hrmode, int n_streams, const int* start_rates, const int* start_bw,
                                        const int* bitrates, const int* bandwidths, int n_frames, int out_stride, int* num_bytes, int* bw_in_force,
                                        uint8_t* flags, int* end_rates, const int32_t* counts)
{
    return enc_plan_rates_host(samplerate, channels, frame_ms, hrmode, n_streams, start_rates, start_bw, bitrates, bandwidths, n_frames, out_stride, num_bytes,
                               bw_in_force, flags, end_rates, counts, 0);
}

/* ---- packed output in device memory (lc3plus_enc_batch_encode_packed) ---- */
LC3_Error lc3plus_enc_batch_encode_packed(lc3plus_batch* b, const void* pcm, int bitdepth, const int32_t* bitrates, const int32_t* bandwidths, int n_frames,
                                          int order, void* out, int64_t out_capacity, int64_t* offsets, int64_t* total, int32_t* num_bytes, uint8_t* flags,
                                          void* hip_stream, int sync)
{
    if (!b || !pcm || !out) return LC3_NULL_ERROR;
    if (!lc3d_pcm_format_ok(bitdepth)) return LC3_ERROR;
    if (placed_refuses(b->placed, 1, bitdepth, NULL)) return LC3_ERROR;
    if (n_frames <= 0 || (order != LC3D_PACK_STREAM_MAJOR && order != LC3D_PACK_FRAME_MAJOR) || out_capacity < 0) return LC3_ERROR;
    if (bandwidths && b->g.hrmode) return LC3_HRMODE_BW_ERROR;
    /* no slot: a rate is refused only where set_bitrate refuses it - the bound on the bytes is the geometry's largest stream-frame */
    const int lim = geom_max_chan_bytes(&b->g) * b->g.channels;
    lc3d_rate_rule r;
    if (enc_rate_rule(&b->g, lim, &r)) return LC3_ERROR;
    const int has = bitrates || bandwidths || b->ragged;      /* (ragged: the plan and tail kernels run whatever the call has, and a stream that did not run keeps a pending reset) */
    if (!has && b->resets_unknown && enc_refresh(b)) return LC3_ERROR;      /* as batch_encode */
    int resets = 0;
    if (enc_words_begin(b, bandwidths != NULL, &resets)) return LC3_ERROR;
    if (lc3hip_encode_packed(b->dev, pcm, bitdepth, n_frames, bitrates, bandwidths, &r, order, out, (long long)out_capacity, (long long*)offsets,
                             (long long*)total, num_bytes, flags, resets, hip_stream, sync)) return LC3_ERROR;
    if (!has) return enc_call_done(b, NULL, NULL, n_frames, hip_stream);         /* nothing of the configuration moved: the call ends as encode() does */
    enc_words_done(b, bitrates != NULL, lim);
    return LC3_OK;
}
/* The offsets of packed output on the host alone (the rule of lc3_pack_offsets_kernel): sizes [n_streams][n_frames] -> offsets [n_streams][n_frames], an
 * exclusive scan of the sizes in `order`; *total (or NULL) their sum; overflow (or NULL) [n_streams][n_frames] LC3D_ENC_FL_PACK_CAP where the frame does
 * not fit capacity, 0 elsewhere. */
LC3_Error lc3plus_plan_packed(const int32_t* sizes, int n_streams, int n_frames, int order, int64_t capacity, int64_t* offsets, int64_t* total, uint8_t* overflow)
{
    if (!sizes || !offsets) return LC3_NULL_ERROR;
    if (n_streams <= 0 || n_frames <= 0 || (order != LC3D_PACK_STREAM_MAJOR && order != LC3D_PACK_FRAME_MAJOR) || capacity < 0) return LC3_ERROR;
    const long long n = (long long)n_streams * n_frames;
    long long off = 0;
    for (long long j = 0; j < n; j++) {
        const long long s = order ? j % n_streams : j / n_frames, t = order ? j / n_streams : j % n_frames;
        const size_t i = (size_t)(s * n_frames + t);
        offsets[i] = off;
        if (overflow) overflow[i] = lc3d_pack_fits(off, sizes[i], capacity) ? 0 : LC3D_ENC_FL_PACK_CAP;
        off += sizes[i];
    }
    if (total) *total = off;
    return LC3_OK;
}

/* debug / stage-parity entry point used by tests: additionally returns one lc3d_trace per channel-frame */
LC3_Error lc3plus_enc_batch_encode_traced(lc3plus_batch* b, const void* pcm, int bitdepth, int n_frames, void* out, int out_stride, void* traces)
{
    return batch_encode(b, pcm, 0, bitdepth, n_frames, out, out_stride, 0, NULL, 1, traces);
}
int lc3plus_trace_sizeof(void) { return (int)sizeof(lc3d_trace); }

float lc3plus_enc_batch_last_kernel_ms(lc3plus_batch* b) { return b ? lc3hip_last_ms(b->dev) : 0.0f; }
int lc3plus_enc_batch_last_status(lc3plus_batch* b, uint8_t* status, int max_entries)
{
    if (!b || !status || max_entries < 0) return -1;
    return lc3hip_last_status(b->dev, status, max_entries);
}
int lc3plus_enc_batch_last_records(lc3plus_batch* b, float* records, int max_words)
{
    if (!b || !records || max_words < 0) return -1;
    return lc3hip_last_records(b->dev, records, max_words);
}
int lc3plus_enc_batch_record_words(void) { return FR_WORDS; }
LC3_Error lc3plus_enc_batch_work_buffer(lc3plus_batch* b, int i, const char** name, void** ptr, size_t* bytes, int* elem)
{
    if (!b || !name || !ptr || !bytes || !elem) return LC3_NULL_ERROR;
    if (lc3hip_wait(b->dev)) return LC3_ERROR;
    return lc3hip_work_buffer(b->dev, i, name, ptr, bytes, elem) ? LC3_ERROR : LC3_OK;
}

size_t lc3plus_enc_batch_state_size(const lc3plus_batch* b) { return b ? lc3hip_state_bytes(b->dev) : 0; }
LC3_Error lc3plus_enc_batch_get_state(lc3plus_batch* b, void* state, size_t size)
{
    if (!b || !state) return LC3_NULL_ERROR;
    return lc3hip_get_state(b->dev, state, size) ? LC3_ERROR : LC3_OK;
}
LC3_Error lc3plus_enc_batch_set_state(lc3plus_batch* b, const void* state, size_t size)
{
    if (!b || !state) return LC3_NULL_ERROR;
    return lc3hip_set_state(b->dev, state, size) ? LC3_ERROR : LC3_OK;
}

size_t lc3plus_enc_batch_stream_state_size(const lc3plus_batch* b) { return b ? stream_blob_bytes(SS_ENC, &b->g) : 0; }
LC3_Error lc3plus_enc_batch_reset_streams(lc3plus_batch* b, const int* streams, int n, const int* bitrates, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    LC3_Error e = stream_list_check(b->n_streams, streams, n);
    if (e) return e;
    const int C = b->g.channels;
    lc3d_chan* cfg = NULL;
    if (bitrates) {                             /* as set_bitrate configures a stream, every rate checked first; the bandwidth is kept */
        if (enc_refresh(b)) return LC3_ERROR;
        cfg = (lc3d_chan*)malloc(sizeof(lc3d_chan) * (size_t)n * C);
        if (!cfg) return LC3_ERROR;
        for (int i = 0; i < n && !e; i++) {
            lc3d_chan* ch = cfg + (size_t)i * C;
            memcpy(ch, b->chans + (size_t)streams[i] * C, sizeof(lc3d_chan) * C);
            e = bitrates[i] <= 0 ? LC3_BITRATE_ERROR : derive_bitrate(&b->g, bitrates[i], ch);
            for (int c = 0; c < C; c++) ch[c].reset_attack = 0;           /* the fresh attack detector is clear already */
        }
        if (e) { free(cfg); return e; }
    }
    uint32_t h[4];
    stream_header(SS_ENC, &b->g, h);
    if (lc3hip_stream_state(b->dev, LC3D_SS_RESET, streams, n, cfg, NULL, 0, h, NULL, hip_stream, sync)) { free(cfg); return LC3_ERROR; }
    if (cfg) {
        for (int i = 0; i < n; i++) {
            memcpy(b->chans + (size_t)streams[i] * C, cfg + (size_t)i * C, sizeof(lc3d_chan) * C);
            b->bitrates[streams[i]] = bitrates[i];
        }
        batch_restride(b);
        free(cfg);
    }
    return LC3_OK;
}
LC3_Error lc3plus_enc_batch_export_streams(lc3plus_batch* b, const int* streams, int n, void* blob, int blob_on_device, void* hip_stream, int sync)
{
    return b ? streams_export(SS_ENC, &b->g, b->n_streams, b->dev, streams, n, blob, blob_on_device, hip_stream, sync) : LC3_NULL_ERROR;
}
LC3_Error lc3plus_enc_batch_import_streams(lc3plus_batch* b, const int* streams, int n, const void* blob, int blob_on_device, uint8_t* status,
                                           void* hip_stream, int sync)
{
    return b ? streams_import(SS_ENC, &b->g, b->n_streams, b->dev, streams, n, blob, blob_on_device, status, hip_stream, sync) : LC3_NULL_ERROR;
}

LC3_Error lc3plus_enc_batch_set_input_ready(lc3plus_batch* b, int ready)
{
    if (!b) return LC3_NULL_ERROR;
    return lc3hip_set_input_ready(b->dev, ready) ? LC3_ERROR : LC3_OK;
}

/* ------------------------------------------------------------------------------------------------ */
/* single-stream drop-in API (R/lc3.h:163-295)                                                       */
/* ------------------------------------------------------------------------------------------------ */
struct LC3_Enc {
    /* R/codec_exe.c is not a pure client of the opaque API: compiled against the reference's own headers it reads encoder->bitrate
     * (:298-299), ->epmode (:310-312) and ->bandwidth (:320) directly, i.e. the words at byte offsets 48, 64 and 144 of the
     * reference's struct (R/setup_enc_lc3.h:65-104 on LP64: five pointers, then ints).  The three fields sit at those offsets here
     * so that the unmodified CLI relinks against this library (`make relink`); the words between them are unused. */
    void* ref_ptr[5];               /*   0 ..  39 */
    int ref_w40[2];                 /*  40 ..  47 */
    int bitrate;                    /*  48 */
    int ref_w52[3];                 /*  52 ..  63 */
    int epmode;                     /*  64 */
    int ref_w68[19];                /*  68 .. 143 */
    int bandwidth;                  /* 144 */
    int ref_w148[7];                /* 148 .. 175: the rest of the reference struct's 176 bytes */
    int lc3_br_set, channels, samplerate, hrmode; float frame_ms;
    geom_t g;
    lc3d_chan ch[MAX_CH];
    lc3plus_batch* batch;           /* batch of one stream, created lazily at the first encode */
    int16_t* stage16; int32_t* stage32; uint8_t* stage_out;
    unsigned magic;
};
_Static_assert(offsetof(struct LC3_Enc, bitrate) == 48 && offsetof(struct LC3_Enc, epmode) == 64 && offsetof(struct LC3_Enc, bandwidth) == 144,
               "fields R/codec_exe.c reads must sit at the reference's offsets");
#define ENC_MAGIC 0x4C433350u

int lc3_version(void) { return LC3_VERSION; }
int lc3_channels_supported(int channels) { return channels >= 1 && channels <= MAX_CH; }
int lc3_samplerate_supported(int samplerate) { return samplerate_ok(samplerate); }

int lc3_enc_get_size(int samplerate, int channels)
{
    if (!lc3_samplerate_supported(samplerate) || !lc3_channels_supported(channels)) return 0;
    return (int)sizeof(struct LC3_Enc);
}

static void enc_drop_device(LC3_Enc* e)
{
    if (e->batch) { lc3plus_enc_batch_destroy(e->batch); e->batch = NULL; }
    free(e->stage16); free(e->stage32); free(e->stage_out); e->stage16 = NULL; e->stage32 = NULL; e->stage_out = NULL;
}

LC3_Error lc3_enc_init(LC3_Enc* e, int samplerate, int channels)
{
    if (e == NULL) return LC3_NULL_ERROR;
    if ((uintptr_t)e % 4 != 0) return LC3_ALIGN_ERROR;
    if (!lc3_samplerate_supported(samplerate)) return LC3_SAMPLERATE_ERROR;
    if (!lc3_channels_supported(channels)) return LC3_CHANNELS_ERROR;
    memset(e, 0, sizeof *e);
    e->magic = ENC_MAGIC; e->channels = channels; e->samplerate = samplerate; e->frame_ms = 10;
    geom_init(&e->g, samplerate, channels);
    geom_update(&e->g);
    return LC3_OK;
}

LC3_Error lc3_enc_set_frame_ms(LC3_Enc* e, float frame_ms)
{
    if (e == NULL) return LC3_NULL_ERROR;
    { int d = (int)ceil(frame_ms * 10); if (d != 25 && d != 50 && d != 100) return LC3_FRAMEMS_ERROR; }
    if (e->lc3_br_set) return LC3_BITRATE_SET_ERROR;
    e->g.dms = (int)(frame_ms * 10); e->g.frame_ms = frame_ms; e->frame_ms = frame_ms;
    geom_update(&e->g);
    enc_drop_device(e);
    return LC3_OK;
}

LC3_Error lc3_enc_set_hrmode(LC3_Enc* e, int hrmode)
{
    if (e == NULL) return LC3_NULL_ERROR;
    if (e->g.fs_in < 48000 && hrmode != 0) return LC3_SAMPLERATE_ERROR;
    e->g.hrmode = hrmode > 0; e->hrmode = e->g.hrmode;
    geom_update(&e->g);
    enc_drop_device(e);
    return LC3_OK;
}

LC3_Error lc3_enc_set_bitrate(LC3_Enc* e, int bitrate)
{
    if (e == NULL) return LC3_NULL_ERROR;
    if (bitrate <= 0) return LC3_BITRATE_ERROR;
    if (e->g.fs_idx == 5 && e->g.hrmode == 0) return LC3_HRMODE_ERROR;
    lc3d_chan tmp[MAX_CH];
    memcpy(tmp, e->ch, sizeof tmp);
    LC3_Error err = derive_bitrate(&e->g, bitrate, tmp);
    if (err) return err;
    memcpy(e->ch, tmp, sizeof tmp);
    e->lc3_br_set = 1; e->bitrate = bitrate;
    if (e->batch) return lc3plus_enc_batch_set_bitrate(e->batch, 0, bitrate);
    return LC3_OK;
}

LC3_Error lc3_enc_set_bandwidth(LC3_Enc* e, int bandwidth)
{
    if (e == NULL) return LC3_NULL_ERROR;
    if (e->g.hrmode == 1) return LC3_HRMODE_BW_ERROR;
    int eff = e->g.fs_in;
    if (e->bandwidth != bandwidth) {
        if (e->g.fs_in > 40000) eff = 40000;
        if (bandwidth * 2 > eff) return LC3_BW_WARNING;
        e->bandwidth = bandwidth;
        for (int c = 0; c < e->channels; c++) {
            e->ch[c].bandwidth = bandwidth; e->ch[c].bw_cut_bin = lc3d_bw_cut_bin(bandwidth, e->g.dms); e->ch[c].bw_index = lc3d_bw_index(bandwidth);
        }
        if (e->batch) return lc3plus_enc_batch_set_bandwidth(e->batch, 0, bandwidth);
    }
    return LC3_OK;
}

int lc3_enc_get_input_samples(const LC3_Enc* e) { return e ? e->g.N : 0; }
int lc3_enc_get_num_bytes(const LC3_Enc* e) { return e ? e->ch[0].nbytes * e->channels : 0; }   /* R/lc3.c:124-129 (sic) */
int lc3_enc_get_delay(const LC3_Enc* e) { return e ? e->g.N - 2 * e->g.la : 0; }
int lc3_enc_get_real_bitrate(const LC3_Enc* e)
{
    if (e == NULL) return 0;
    if (!e->lc3_br_set) return LC3_BITRATE_UNSET_ERROR;
    int tot = 0;
    for (int c = 0; c < e->channels; c++) tot += e->ch[c].nbytes;
    int br = (tot * 80000) / e->g.dms;
    if (e->g.fs_in == 44100) { int rem = br % 480; br = ((br - rem) / 480) * 441 + (rem * 441) / 480; }
    return br;
}

LC3_Error lc3_enc_fl(LC3_Enc* e, void** input_samples, int bitdepth, void* output_bytes, int* num_bytes)
{
    if (!e || !input_samples || !output_bytes || !num_bytes) return LC3_NULL_ERROR;
    for (int c = 0; c < e->channels; c++) if (input_samples[c] == NULL) return LC3_NULL_ERROR;
    if (bitdepth != 16 && bitdepth != 24 && bitdepth != 32) return LC3_ERROR;
    if (!e->lc3_br_set) return LC3_BITRATE_UNSET_ERROR;
    const int N = e->g.N, C = e->channels;
    if (!e->batch) {
        LC3_Error err = lc3plus_enc_batch_create(&e->batch, 1, e->g.fs_in, C, e->g.frame_ms, e->g.hrmode, &e->bitrate, -1);
        if (err) return err == LC3_BITRATE_ERROR ? err : LC3_ERROR;
        if (e->bandwidth) lc3plus_enc_batch_set_bandwidth(e->batch, 0, e->bandwidth);
        e->stage16 = (int16_t*)malloc(sizeof(int16_t) * C * LC3D_MAX_N);
        e->stage32 = (int32_t*)malloc(sizeof(int32_t) * C * LC3D_MAX_N);
        e->stage_out = (uint8_t*)malloc(LC3_MAX_BYTES);
        if (!e->stage16 || !e->stage32 || !e->stage_out) { enc_drop_device(e); return LC3_ERROR; }
    }
    const void* pcm;
    if (bitdepth == 16) { for (int c = 0; c < C; c++) memcpy(e->stage16 + c * N, input_samples[c], sizeof(int16_t) * N); pcm = e->stage16; }
    else { for (int c = 0; c < C; c++) memcpy(e->stage32 + c * N, input_samples[c], sizeof(int32_t) * N); pcm = e->stage32; }
    const int nb = lc3plus_enc_batch_num_bytes(e->batch, 0);
    LC3_Error err = lc3plus_enc_batch_encode(e->batch, pcm, 0, bitdepth, 1, output_bytes, nb, 0, NULL, 1);
    if (err) return err;
    *num_bytes = nb;
    return LC3_OK;
}
LC3_Error lc3_enc16(LC3_Enc* e, int16_t** in, void* out, int* nb) { return lc3_enc_fl(e, (void**)in, 16, out, nb); }
LC3_Error lc3_enc24(LC3_Enc* e, int32_t** in, void* out, int* nb) { return lc3_enc_fl(e, (void**)in, 24, out, nb); }
LC3_Error lc3_enc32(LC3_Enc* e, int32_t** in, void* out, int* nb) { return lc3_enc_fl(e, (void**)in, 32, out, nb); }

LC3_Error lc3_free_encoder_structs(LC3_Enc* e)
{
    if (!e) return LC3_NULL_ERROR;
    if (e->magic == ENC_MAGIC) enc_drop_device(e);
    return LC3_OK;
}
LC3_Error lc3_enc_free_memory(LC3_Enc* e)
{
    if (!e) return LC3_NULL_ERROR;
    lc3_free_encoder_structs(e);
    free(e);
    return LC3_OK;
}

/* lc3plus_enc_* aliases (north-star wording) */
LC3_Error lc3plus_enc_init(LC3_Enc* e, int sr, int ch) { return lc3_enc_init(e, sr, ch); }
LC3_Error lc3plus_enc_set_frame_ms(LC3_Enc* e, float ms) { return lc3_enc_set_frame_ms(e, ms); }
LC3_Error lc3plus_enc_set_hrmode(LC3_Enc* e, int hr) { return lc3_enc_set_hrmode(e, hr); }
LC3_Error lc3plus_enc_set_bitrate(LC3_Enc* e, int br) { return lc3_enc_set_bitrate(e, br); }
LC3_Error lc3plus_enc16(LC3_Enc* e, int16_t** in, void* out, int* nb) { return lc3_enc16(e, in, out, nb); }
int lc3plus_enc_get_size(int sr, int ch) { return lc3_enc_get_size(sr, ch); }


/* ================================================================================================ */
/* decoder: lc3_dec_* drop-in API and the batched form                          */
/* ================================================================================================ */
/* R/setup_dec_lc3.c:203-299 (update_dec_bitrate) for one channel */
static LC3_Error derive_dchan(const geom_t* g, int nbytes, lc3d_dchan* d)
{
    int min_b = 20, max_b = 400;                                          /* R/defines.h MIN_NBYTES / MAX_NBYTES */
    if (g->hrmode) {
        switch (g->dms) {
        case 25:  max_b = 210; if (g->fs == 48000) min_b = 54;  else if (g->fs == 96000) min_b = 62;  else return LC3_HRMODE_ERROR; break;
        case 50:  max_b = 375; if (g->fs == 48000) min_b = 93;  else if (g->fs == 96000) min_b = 109; else return LC3_HRMODE_ERROR; break;
        case 100: max_b = 625; if (g->fs == 48000) min_b = 156; else if (g->fs == 96000) min_b = 187; else return LC3_HRMODE_ERROR; break;
        default: return LC3_HRMODE_ERROR;
        }
    }
    if (nbytes < min_b || nbytes > max_b) return LC3_NUMBYTES_ERROR;
    const int total_bits = nbytes << 3;
    d->nbytes = nbytes;
    d->lpc_weighting = total_bits < 480;
    d->gg_off = -(IMIN(115, total_bits / (10 * (g->fs_idx + 1))) + 105 + 5 * (g->fs_idx + 1));
    int tb = total_bits;
    if (g->dms == 25) { d->lpc_weighting = total_bits < 120; tb = (int)(total_bits * 4.0 * (1.0 - 0.4)); }
    if (g->dms == 50) { d->lpc_weighting = total_bits < 240; tb = total_bits * 2 - 160; }
    if (g->N > 40 * ((float)g->dms / 10.0)) { d->N_red_tns = (int)(40 * ((float)g->dms / 10.0)); d->fs_red_tns = 40000; }
    else { d->N_red_tns = g->N; d->fs_red_tns = g->fs; }
    const int k = (g->fs_idx - 1) * 80;
    if (tb < 400 + k)      { d->ltpf_beta = 0.4f;  d->ltpf_beta_idx = 0; }
    else if (tb < 480 + k) { d->ltpf_beta = 0.35f; d->ltpf_beta_idx = 1; }
    else if (tb < 560 + k) { d->ltpf_beta = 0.3f;  d->ltpf_beta_idx = 2; }
    else if (tb < 640 + k) { d->ltpf_beta = 0.25f; d->ltpf_beta_idx = 3; }
    else                   { d->ltpf_beta = 0;     d->ltpf_beta_idx = -1; }
    if (g->hrmode == 1) { d->ltpf_beta = 0; d->ltpf_beta_idx = -1; }
    return LC3_OK;
}

/* split of a stream-frame of num_bytes over the channels (R/dec_lc3_fl.c:148) and the payload offsets */
static LC3_Error derive_dstream(const geom_t* g, int num_bytes, lc3d_dchan* d /* [channels] */)
{
    int off = 0;
    for (int c = 0; c < g->channels; c++) {
        LC3_Error e = derive_dchan(g, num_bytes / g->channels + (c < (num_bytes % g->channels)), d + c);
        if (e) return e;
        d[c].in_off = off; off += d[c].nbytes;
    }
    return LC3_OK;
}

/* test hook: what a channel of nbytes bytes is configured with, without a device - derive_chan's words (encoder) and derive_dchan's (decoder), the rules
 * every kernel's per-size behaviour comes from.  out[10]: total_bits, target_bits_init, lpc_weighting, ltpf_enable, gg_off, attack_handling, reg_bits,
 * and the decoder's lpc_weighting, gg_off, ltpf_beta_idx.  LC3_NUMBYTES_ERROR for a size the decoder refuses. */
LC3_Error lc3plus_plan_chan(int samplerate, float frame_ms, int hrmode, int nbytes, int* out)
{
    if (!out) return LC3_NULL_ERROR;
    LC3_Error e = geom_check(samplerate, 1, frame_ms, hrmode, 0);
    if (e) return e;
    geom_t g;
    geom_fill(&g, samplerate, 1, frame_ms, hrmode, 0);
    lc3d_chan s; lc3d_dchan d;
    memset(&s, 0, sizeof s); memset(&d, 0, sizeof d);
    e = derive_dchan(&g, nbytes, &d);
    if (e) return e;
    derive_chan(&g, nbytes, &s);
    const int v[10] = {s.total_bits, s.target_bits_init, s.lpc_weighting, s.ltpf_enable, s.gg_off, s.attack_handling, s.reg_bits,
                       d.lpc_weighting, d.gg_off, d.ltpf_beta_idx};
    memcpy(out, v, sizeof v);
    return LC3_OK;
}

/* per-frame sizes: the configuration of every channel byte count 0 .. max, from derive_dchan (entry 0 and the sizes it rejects: zeroed, which is what a
 * channel created without a size has).  An entry is valid where its nbytes equals its index and is not 0. */
static lc3d_dchan* dec_build_table(const geom_t* g, int* n)
{
    *n = geom_max_chan_bytes(g) + 1;
    lc3d_dchan* tab = (lc3d_dchan*)calloc((size_t)*n, sizeof(lc3d_dchan));
    if (!tab) return NULL;
    for (int k = 1; k < *n; k++) if (derive_dchan(g, k, &tab[k])) memset(&tab[k], 0, sizeof tab[k]);
    return tab;
}

/* The per-frame size rule of lc3plus_dec_batch_decode_sizes (R/dec_lc3_fl.c:134-163 per stream): a frame is lost where bfi is 1 or its size is 0; a good
 * frame's size configures its channels, a lost one keeps the size of the stream's last good frame (start[s] before the first).  Validates every good size
 * (geometry limits through the table, <= in_stride) and every flag (0 or 1) before anything is written.  Out: eff [s][t] the size each frame is configured
 * with, lost [s][t] 0 / 1, end[s] the size after the call, *max_chan the largest channel frame that is not lost (0: none). */
static LC3_Error dec_plan_sizes(const geom_t* g, const lc3d_dchan* tab, int tab_n, int n_streams, const int* start, const int* num_bytes, const uint8_t* bfi,
                                int n_frames, int in_stride, uint16_t* eff, uint8_t* lost, int* end, int* max_chan)
{
    const int C = g->channels;
    const size_t n = (size_t)n_streams * n_frames;
    int mx = 0;
    for (size_t i = 0; i < n; i++) {
        const int nb = num_bytes[i];
        const int k = lc3d_dec_frame_class(nb, bfi ? bfi[i] : 0, in_stride, tab, tab_n, C);
        if (k == LC3D_FRAME_BAD_FLAG) return LC3_ERROR;
        if (k == LC3D_FRAME_BAD_SIZE) return LC3_NUMBYTES_ERROR;
        if (k == LC3D_FRAME_GOOD && (nb + C - 1) / C > mx) mx = (nb + C - 1) / C;
    }
    for (int s = 0; s < n_streams; s++) {
        int cur = start[s];
        for (int t = 0; t < n_frames; t++) {
            const size_t i = (size_t)s * n_frames + t;
            const int l = (bfi && bfi[i]) || num_bytes[i] == 0;
            if (!l) cur = num_bytes[i];
            eff[i] = (uint16_t)cur; lost[i] = (uint8_t)l;
        }
        end[s] = cur;
    }
    *max_chan = mx;
    return LC3_OK;
}

/* The rule of lc3plus_dec_batch_decode_sizes_device on the host (on the device: lc3_dec_plan_sizes_kernel and lc3_dec_sizes_tail_kernel): as
 * dec_plan_sizes, except that a size or flag the host call refuses does not fail the call - the frame is lost, marked in invalid[s][t], and does not
 * move the carry.  Nothing is refused.
 * The same loop serves lc3plus_dec_batch_decode_packed, whose frames are classified by offsets, capacity and max_bytes in place of in_stride: `cls` gives
 * the class of frame i (LC3D_FRAME_*) from the call's arguments `a`. */
typedef struct {
    const lc3d_dchan* tab; int tab_n, channels; const int* num_bytes; const uint8_t* bfi;
    int in_stride;                                                       /* slots (dec_class_slot) */
    const int64_t* offsets; int64_t capacity; int max_bytes;             /* packed (dec_class_packed) */
} dec_class_args;
static int dec_class_slot(const dec_class_args* a, size_t i)
{
    return lc3d_dec_frame_class(a->num_bytes[i], a->bfi ? a->bfi[i] : 0, a->in_stride, a->tab, a->tab_n, a->channels);
}
static int dec_class_packed(const dec_class_args* a, size_t i)
{
    return lc3d_dec_frame_class_packed(a->num_bytes[i], a->bfi ? a->bfi[i] : 0, (long long)a->offsets[i], (long long)a->capacity, a->max_bytes, a->tab, a->tab_n,
                                       a->channels);
}
static void dec_plan_lenient(int (*cls)(const dec_class_args*, size_t), const dec_class_args* a, int n_streams, const int* start, int n_frames, uint16_t* eff,
                             uint8_t* lost, uint8_t* invalid, int* end, int* max_chan)
{
    const int C = a->channels;
    int mx = 0;
    for (int s = 0; s < n_streams; s++) {
        int cur = start[s];
        for (int t = 0; t < n_frames; t++) {
            const size_t i = (size_t)s * n_frames + t;
            const int k = cls(a, i);
            if (k == LC3D_FRAME_GOOD) { cur = a->num_bytes[i]; if ((cur + C - 1) / C > mx) mx = (cur + C - 1) / C; }
            eff[i] = (uint16_t)cur; lost[i] = k != LC3D_FRAME_GOOD; invalid[i] = k >= LC3D_FRAME_BAD_FLAG;
        }
        end[s] = cur;
    }
    *max_chan = mx;
}

struct lc3plus_dec_batch {
    geom_t g; int n_streams;
    lc3d_dchan* chans;               /* [n_streams * channels] host mirror */
    int chans_stale;                 /* a call with sizes in device memory has changed the configuration on the device: dec_refresh before reading chans */
    void* dev;
    lc3d_dchan* tab; int tab_n;      /* dec_build_table, also on the device */
    uint16_t* eff; size_t eff_cap; uint8_t* lost; size_t lost_cap; int* sz;      /* per-frame sizes: host buffers of dec_plan_sizes, grown as needed */
    int dry;                         /* as lc3plus_batch.dry: the call returns behind its checks */
    int placed;                      /* as lc3plus_batch.placed (lc3plus_dec_batch_set_pcm_placement) */
    int ragged;                      /* lc3plus_dec_batch_set_frame_counts is on: only the calls with sizes in device memory decode, the others refuse */
};
/* all the packet layer sees of a decoder batch (lc3_batch_view.h) */
lc3host_view lc3host_dec_view(const lc3plus_dec_batch* b) { const lc3host_view v = {b->dev, 1, b->n_streams, b->g.channels, b->g.ylen}; return v; }

/* the geometry of a decoder batch, or the error create gives for it; no device */
static LC3_Error dec_batch_geometry(geom_t* g, int n_streams, int samplerate, int channels, float frame_ms, int hrmode)
{
    if (n_streams <= 0) return LC3_ERROR;
    const LC3_Error e = geom_check(samplerate, channels, frame_ms, hrmode, 1);
    if (e) return e;
    geom_fill(g, samplerate, channels, frame_ms, hrmode, 1);
    if (!geom_supported(g)) {
        fprintf(stderr, "lc3plus_hip: decoding %d Hz / %.1f ms%s is not built into the gfx950 kernels yet\n", samplerate, frame_ms, hrmode ? " hr" : "");
        return LC3_ERROR;
    }
    return LC3_OK;
}

LC3_Error lc3plus_dec_batch_create(lc3plus_dec_batch** out, int n_streams, int samplerate, int channels, float frame_ms, int hrmode,
                                   const int* num_bytes, int device)
{
    if (!out) return LC3_NULL_ERROR;
    *out = NULL;
    geom_t g;
    { LC3_Error e = dec_batch_geometry(&g, n_streams, samplerate, channels, frame_ms, hrmode); if (e) return e; }
    lc3plus_dec_batch* b = (lc3plus_dec_batch*)calloc(1, sizeof *b);
    if (!b) return LC3_ERROR;
    b->g = g;
    b->n_streams = n_streams;
    b->chans = (lc3d_dchan*)calloc((size_t)n_streams * channels, sizeof(lc3d_dchan));
    if (!b->chans) { free(b); return LC3_ERROR; }
    if (num_bytes)
        for (int i = 0; i < n_streams; i++) {
            LC3_Error e = derive_dstream(&b->g, num_bytes[i], b->chans + (size_t)i * channels);
            if (e) { free(b->chans); free(b); return e; }
        }
    lc3d_plan* plan = (lc3d_plan*)malloc(sizeof *plan);
    if (!plan) { free(b->chans); free(b); return LC3_ERROR; }
    build_plan(&b->g, plan);
    float st[DST_WORDS];
    dec_init_state(st);
    int rc = lc3hip_dec_create(&b->dev, plan, st, n_streams, device);
    free(plan);
    if (!rc) rc = lc3hip_dec_upload_chans(b->dev, b->chans, 0, n_streams * channels);
    if (!rc) { b->tab = dec_build_table(&b->g, &b->tab_n); rc = !b->tab || lc3hip_dec_upload_table(b->dev, b->tab, b->tab_n); }
    if (rc) { if (b->dev) lc3hip_dec_destroy(b->dev); free(b->tab); free(b->chans); free(b); return LC3_ERROR; }
    *out = b;
    return LC3_OK;
}

size_t lc3plus_dec_batch_state_size(const lc3plus_dec_batch* b) { return b ? lc3hip_dec_state_bytes(b->dev) : 0; }
LC3_Error lc3plus_dec_batch_get_state(lc3plus_dec_batch* b, void* state, size_t size)
{
    if (!b || !state) return LC3_NULL_ERROR;
    return lc3hip_dec_get_state(b->dev, state, size) ? LC3_ERROR : LC3_OK;
}
LC3_Error lc3plus_dec_batch_set_state(lc3plus_dec_batch* b, const void* state, size_t size)
{
    if (!b || !state) return LC3_NULL_ERROR;
    return lc3hip_dec_set_state(b->dev, state, size) ? LC3_ERROR : LC3_OK;
}

LC3_Error lc3plus_dec_batch_destroy(lc3plus_dec_batch* b)
{
    if (!b) return LC3_NULL_ERROR;
    lc3hip_dec_destroy(b->dev);
    free(b->tab); free(b->eff); free(b->lost); free(b->sz);
    free(b->chans); free(b);
    return LC3_OK;
}

int lc3plus_dec_batch_output_samples(const lc3plus_dec_batch* b) { return b ? b->g.N : 0; }
int lc3plus_dec_batch_delay(const lc3plus_dec_batch* b) { return b ? b->g.N - 2 * b->g.la : 0; }
/* Brings the host mirror of the configuration back after calls with sizes in device memory: waits for the batch's last call and downloads it, once. */
static LC3_Error dec_refresh(lc3plus_dec_batch* b)
{
    if (!b->chans_stale) return LC3_OK;
    if (lc3hip_dec_download_chans(b->dev, b->chans)) return LC3_ERROR;
    b->chans_stale = 0;
    return LC3_OK;
}
int lc3plus_dec_batch_num_bytes(const lc3plus_dec_batch* b, int stream)
{
    if (!b || stream < 0 || stream >= b->n_streams) return 0;
    /* (the mirror is a cache of the device's configuration: refreshing it leaves the batch as it was) */
    if (dec_refresh((lc3plus_dec_batch*)b)) return 0;
    int n = 0;
    for (int c = 0; c < b->g.channels; c++) n += b->chans[stream * b->g.channels + c].nbytes;
    return n;
}

/* frame size change of one stream between decode() calls: what R/dec_lc3_fl.c:149-155 does when num_bytes changes */
LC3_Error lc3plus_dec_batch_set_num_bytes(lc3plus_dec_batch* b, int stream, int num_bytes)
{
    if (!b) return LC3_NULL_ERROR;
    if (stream < 0 || stream >= b->n_streams) return LC3_ERROR;
    lc3d_dchan tmp[MAX_CH];
    memset(tmp, 0, sizeof tmp);
    LC3_Error e = derive_dstream(&b->g, num_bytes, tmp);
    if (e) return e;
    if (dec_refresh(b)) return LC3_ERROR;
    memcpy(b->chans + (size_t)stream * b->g.channels, tmp, sizeof(lc3d_dchan) * b->g.channels);
    return lc3hip_dec_upload_chans(b->dev, tmp, stream * b->g.channels, b->g.channels) ? LC3_ERROR : LC3_OK;
}

static LC3_Error dec_batch_decode(lc3plus_dec_batch* b, const void* frames, int frames_on_device, int in_stride, const uint8_t* bfi, int n_frames,
                                  void* pcm, int pcm_on_device, int bps, uint8_t* status, void* hip_stream, int sync, void* traces)
{
    if (!b || !frames || !pcm) return LC3_NULL_ERROR;
    if (!lc3d_pcm_format_ok(bps)) return LC3_ERROR;
    if (placed_refuses(b->placed, pcm_on_device, bps, traces)) return LC3_ERROR;
    if (b->ragged) return LC3_ERROR;                                 /* per-stream frame counts are read by the device-size calls alone; nothing is touched here */
    if (traces && !pcm_format_plain(bps)) return LC3_ERROR;          /* the traced call writes the integer formats in the default layout only */
    if (n_frames <= 0) return LC3_ERROR;
    if (dec_refresh(b)) return LC3_ERROR;
    for (int i = 0; i < b->n_streams; i++) if (lc3plus_dec_batch_num_bytes(b, i) > in_stride) return LC3_NUMBYTES_ERROR;
    DRY_STOP(b, DRY_ALL, LC3_OK);
    return lc3hip_dec_decode(b->dev, frames, frames_on_device, in_stride, bfi, NULL, 0, n_frames, pcm, pcm_on_device, bps, status, hip_stream, sync, traces)
               ? LC3_ERROR : LC3_OK;
}
LC3_Error lc3plus_dec_batch_decode_sizes(lc3plus_dec_batch* b, const void* frames, int frames_on_device, int in_stride, const int* num_bytes,
                                         const uint8_t* bfi, int n_frames, void* pcm, int pcm_on_device, int bps, uint8_t* status, void* hip_stream, int sync)
{
    if (!b || !frames || !pcm || !num_bytes) return LC3_NULL_ERROR;
    if (!lc3d_pcm_format_ok(bps)) return LC3_ERROR;
    if (placed_refuses(b->placed, pcm_on_device, bps, NULL)) return LC3_ERROR;
    if (b->ragged) return LC3_ERROR;                                 /* as in dec_batch_decode */
    if (n_frames <= 0) return LC3_ERROR;
    if (dec_refresh(b)) return LC3_ERROR;
    const size_t n = (size_t)b->n_streams * n_frames;
    b->eff = (uint16_t*)scratch_grow(b->eff, &b->eff_cap, n, sizeof(uint16_t));
    b->lost = (uint8_t*)scratch_grow(b->lost, &b->lost_cap, n, 1);
    if (!b->eff || !b->lost) return LC3_ERROR;
    if (!b->sz) { b->sz = (int*)malloc(2 * sizeof(int) * (size_t)b->n_streams); if (!b->sz) return LC3_ERROR; }
    int* start = b->sz; int* end = b->sz + b->n_streams;
    for (int i = 0; i < b->n_streams; i++) start[i] = lc3plus_dec_batch_num_bytes(b, i);
    int max_chan = 0;
    LC3_Error e = dec_plan_sizes(&b->g, b->tab, b->tab_n, b->n_streams, start, num_bytes, bfi, n_frames, in_stride, b->eff, b->lost, end, &max_chan);
    if (e) return e;
    DRY_STOP(b, DRY_ALL, LC3_OK);
    /* the kernels take the size of every good frame and 0 for a lost one: the parser reads nothing of a lost frame's slot, and the concealment kernel
     * carries the last good configuration from frame to frame (from the stream's configuration before the call), as dec_plan_sizes does here */
    for (size_t i = 0; i < n; i++) if (b->lost[i]) b->eff[i] = 0;
    /* the call is ordered and synchronous (it passes flags), and no kernel of it reads the per-stream configuration: that is brought to the last good
     * size of every stream after it */
    if (lc3hip_dec_decode(b->dev, frames, frames_on_device, in_stride, b->lost, b->eff, max_chan, n_frames, pcm, pcm_on_device, bps, status, hip_stream, sync, NULL))
        return LC3_ERROR;
    int changed = 0;
    for (int i = 0; i < b->n_streams; i++) {
        if (end[i] == start[i]) continue;
        lc3d_dchan* d = b->chans + (size_t)i * b->g.channels;
        for (int c = 0, off = 0; c < b->g.channels; c++) {
            d[c] = b->tab[end[i] / b->g.channels + (c < end[i] % b->g.channels)];
            d[c].in_off = off; off += d[c].nbytes;
        }
        changed = 1;
    }
    if (changed && lc3hip_dec_upload_chans(b->dev, b->chans, 0, b->n_streams * b->g.channels)) return LC3_ERROR;
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_decode_sizes_device(lc3plus_dec_batch* b, const void* frames, int in_stride, const int32_t* num_bytes, const uint8_t* bfi,
                                                int n_frames, void* pcm, int bps, uint8_t* status, void* hip_stream, int sync)
{
    if (!b || !frames || !pcm || !num_bytes) return LC3_NULL_ERROR;
    if (!lc3d_pcm_format_ok(bps)) return LC3_ERROR;
    if (placed_refuses(b->placed, 1, bps, NULL)) return LC3_ERROR;
    if (n_frames <= 0 || in_stride <= 0) return LC3_ERROR;
    /* the sizes, the carry and the configuration after the call are on the device only: the host mirror is read back by the next host-side reader */
    if (lc3hip_dec_decode_dsizes(b->dev, frames, in_stride, num_bytes, bfi, n_frames, pcm, bps, status, hip_stream, sync)) return LC3_ERROR;
    b->chans_stale = 1;
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_decode_packed(lc3plus_dec_batch* b, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes,
                                          int max_frame_bytes, const uint8_t* bfi, int n_frames, void* pcm, int bps, uint8_t* status, void* hip_stream, int sync)
{
    if (!b || !frames || !pcm || !num_bytes || !offsets) return LC3_NULL_ERROR;
    if (!lc3d_pcm_format_ok(bps)) return LC3_ERROR;
    if (placed_refuses(b->placed, 1, bps, NULL)) return LC3_ERROR;
    if (n_frames <= 0 || max_frame_bytes <= 0 || frames_capacity < 0) return LC3_ERROR;
    if (lc3hip_dec_decode_packed(b->dev, frames, (long long)frames_capacity, (const long long*)offsets, num_bytes, max_frame_bytes, bfi, n_frames, pcm, bps,
                                 status, hip_stream, sync)) return LC3_ERROR;
    b->chans_stale = 1;
    return LC3_OK;
}
size_t lc3plus_dec_batch_stream_state_size(const lc3plus_dec_batch* b) { return b ? stream_blob_bytes(SS_DEC, &b->g) : 0; }
LC3_Error lc3plus_dec_batch_reset_streams(lc3plus_dec_batch* b, const int* streams, int n, const int* num_bytes, void* hip_stream, int sync)
{
    if (!b) return LC3_NULL_ERROR;
    LC3_Error e = stream_list_check(b->n_streams, streams, n);
    if (e) return e;
    const int C = b->g.channels;
    lc3d_dchan* cfg = NULL;
    if (num_bytes) {                            /* as set_num_bytes configures a stream, every size checked first */
        cfg = (lc3d_dchan*)calloc((size_t)n * C, sizeof(lc3d_dchan));
        if (!cfg) return LC3_ERROR;
        for (int i = 0; i < n && !e; i++) e = derive_dstream(&b->g, num_bytes[i], cfg + (size_t)i * C);
        if (e) { free(cfg); return e; }
    }
    uint32_t h[4];
    stream_header(SS_DEC, &b->g, h);
    /* no dec_refresh: the configuration is written on the device, in order; a stale host copy stays stale and is read back by the next host-side reader */
    if (lc3hip_dec_stream_state(b->dev, LC3D_SS_RESET, streams, n, cfg, NULL, 0, h, NULL, hip_stream, sync)) { free(cfg); return LC3_ERROR; }
    if (cfg && !b->chans_stale)
        for (int i = 0; i < n; i++) memcpy(b->chans + (size_t)streams[i] * C, cfg + (size_t)i * C, sizeof(lc3d_dchan) * C);
    free(cfg);
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_export_streams(lc3plus_dec_batch* b, const int* streams, int n, void* blob, int blob_on_device, void* hip_stream, int sync)
{
    return b ? streams_export(SS_DEC, &b->g, b->n_streams, b->dev, streams, n, blob, blob_on_device, hip_stream, sync) : LC3_NULL_ERROR;
}
LC3_Error lc3plus_dec_batch_import_streams(lc3plus_dec_batch* b, const int* streams, int n, const void* blob, int blob_on_device, uint8_t* status,
                                           void* hip_stream, int sync)
{
    return b ? streams_import(SS_DEC, &b->g, b->n_streams, b->dev, streams, n, blob, blob_on_device, status, hip_stream, sync) : LC3_NULL_ERROR;
}
/* test hooks of the lifecycle rules, without a device: the index-list rule; the blob header of a geometry (decoder != 0: the decoder's; the checks of the
 * batch's create, LC3_ERROR where the kernels do not support the geometry); the header check of an import */
LC3_Error lc3plus_stream_list_check(int n_streams, const int* streams, int n) { return stream_list_check(n_streams, streams, n); }
LC3_Error lc3plus_stream_state_header(int decoder, int samplerate, int channels, float frame_ms, int hrmode, uint32_t* header)
{
    if (!header) return LC3_NULL_ERROR;
    const LC3_Error e = geom_check(samplerate, channels, frame_ms, hrmode, decoder != 0);
    if (e) return e;
    geom_t g;
    geom_fill(&g, samplerate, channels, frame_ms, hrmode, decoder != 0);
    if (!geom_supported(&g)) return LC3_ERROR;
    stream_header(decoder ? SS_DEC : SS_ENC, &g, header);
    return LC3_OK;
}
int lc3plus_stream_header_ok(const uint32_t* header, const void* blob) { return header && blob && stream_header_ok(header, blob); }

/* test hooks: dec_plan_sizes and dec_plan_lenient for a geometry, without a device (the batch builds the same table at create) */
static LC3_Error dec_hook_table(int samplerate, int channels, float frame_ms, int hrmode, geom_t* g, lc3d_dchan** tab, int* tab_n)
{
    const LC3_Error e = geom_check_io(samplerate, channels);               /* (the frame length and hrmode are the caller's to get right) */
    if (e) return e;
    geom_fill(g, samplerate, channels, frame_ms, hrmode, 1);
    *tab = dec_build_table(g, tab_n);
    return *tab ? LC3_OK : LC3_ERROR;
}
LC3_Error lc3plus_dec_plan_sizes(int samplerate, int channels, float frame_ms, int hrmode, int n_streams, const int* start, const int* num_bytes,
                                 const uint8_t* bfi, int n_frames, int in_stride, uint16_t* eff, uint8_t* lost, int* end, int* max_chan)
{
    if (!start || !num_bytes || !eff || !lost || !end || !max_chan) return LC3_NULL_ERROR;
    geom_t g; lc3d_dchan* tab = NULL; int tab_n = 0;
    LC3_Error e = dec_hook_table(samplerate, channels, frame_ms, hrmode, &g, &tab, &tab_n);
    if (e) return e;
    e = dec_plan_sizes(&g, tab, tab_n, n_streams, start, num_bytes, bfi, n_frames, in_stride, eff, lost, end, max_chan);
    free(tab);
    return e;
}
LC3_Error lc3plus_dec_plan_sizes_lenient(int samplerate, int channels, float frame_ms, int hrmode, int n_streams, const int* start, const int* num_bytes,
                                         const uint8_t* bfi, int n_frames, int in_stride, uint16_t* eff, uint8_t* lost, uint8_t* invalid, int* end, int* max_chan)
{
    if (!start || !num_bytes || !eff || !lost || !invalid || !end || !max_chan) return LC3_NULL_ERROR;
    geom_t g; lc3d_dchan* tab = NULL; int tab_n = 0;
    LC3_Error e = dec_hook_table(samplerate, channels, frame_ms, hrmode, &g, &tab, &tab_n);
    if (e) return e;
    const dec_class_args a = {tab, tab_n, g.channels, num_bytes, bfi, in_stride, NULL, 0, 0};
    dec_plan_lenient(dec_class_slot, &a, n_streams, start, n_frames, eff, lost, invalid, end, max_chan);
    free(tab);
    return LC3_OK;
}
LC3_Error lc3plus_dec_plan_packed_lenient(int samplerate, int channels, float frame_ms, int hrmode, int n_streams, const int* start, const int* num_bytes,
                                          const int64_t* offsets, int64_t frames_capacity, int max_frame_bytes, const uint8_t* bfi, int n_frames, uint16_t* eff,
                                          uint8_t* lost, uint8_t* invalid, int* end, int* max_chan)
{
    if (!start || !num_bytes || !offsets || !eff || !lost || !invalid || !end || !max_chan) return LC3_NULL_ERROR;
    if (max_frame_bytes <= 0) return LC3_ERROR;
    geom_t g; lc3d_dchan* tab = NULL; int tab_n = 0;
    LC3_Error e = dec_hook_table(samplerate, channels, frame_ms, hrmode, &g, &tab, &tab_n);
    if (e) return e;
    const dec_class_args a = {tab, tab_n, g.channels, num_bytes, bfi, 0, offsets, frames_capacity, max_frame_bytes};
    dec_plan_lenient(dec_class_packed, &a, n_streams, start, n_frames, eff, lost, invalid, end, max_chan);
    free(tab);
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_decode(lc3plus_dec_batch* b, const void* frames, int frames_on_device, int in_stride, const uint8_t* bfi, int n_frames,
                                   void* pcm, int pcm_on_device, int bps, uint8_t* status, void* hip_stream, int sync)
{
    return dec_batch_decode(b, frames, frames_on_device, in_stride, bfi, n_frames, pcm, pcm_on_device, bps, status, hip_stream, sync, NULL);
}
/* test hook: per channel-stream per frame stage traces (lc3d_dec_trace), host pointers only */
LC3_Error lc3plus_dec_batch_decode_traced(lc3plus_dec_batch* b, const void* frames, int in_stride, const uint8_t* bfi, int n_frames, void* pcm, int bps,
                                          uint8_t* status, void* traces)
{
    return dec_batch_decode(b, frames, 0, in_stride, bfi, n_frames, pcm, 0, bps, status, NULL, 1, traces);
}
int lc3plus_dec_trace_sizeof(void) { return (int)sizeof(lc3d_dec_trace); }
float lc3plus_dec_batch_last_kernel_ms(lc3plus_dec_batch* b) { return b ? lc3hip_dec_last_ms(b->dev) : 0.0f; }
LC3_Error lc3plus_dec_batch_work_buffer(lc3plus_dec_batch* b, int i, const char** name, void** ptr, size_t* bytes, int* elem)
{
    if (!b || !name || !ptr || !bytes || !elem) return LC3_NULL_ERROR;
    if (lc3hip_dec_wait(b->dev)) return LC3_ERROR;
    return lc3hip_dec_work_buffer(b->dev, i, name, ptr, bytes, elem) ? LC3_ERROR : LC3_OK;
}
LC3_Error lc3plus_dec_batch_set_input_ready(lc3plus_dec_batch* b, int ready)
{
    if (!b) return LC3_NULL_ERROR;
    return lc3hip_dec_set_input_ready(b->dev, ready) ? LC3_ERROR : LC3_OK;
}
LC3_Error lc3plus_dec_batch_set_pcm_placement(lc3plus_dec_batch* b, const int64_t* offsets, int64_t capacity)
{
    if (!b) return LC3_NULL_ERROR;
    if (capacity < 0) return LC3_ERROR;
    if (lc3hip_dec_set_pcm_placement(b->dev, (const long long*)offsets, (long long)capacity)) return LC3_ERROR;
    b->placed = offsets != NULL;
    return LC3_OK;
}
LC3_Error lc3plus_dec_batch_set_frame_counts(lc3plus_dec_batch* b, const int32_t* counts)
{
    if (!b) return LC3_NULL_ERROR;
    if (lc3hip_dec_set_frame_counts(b->dev, counts)) return LC3_ERROR;
    b->ragged = counts != NULL;
    return LC3_OK;
}
LC3_Error lc3plus_dec_plan_counts(const int32_t* counts, int n_streams, int n_frames, int32_t* effective)
{
    if (n_streams < 0 || n_frames <= 0) return LC3_ERROR;
    if (n_streams > 0 && (!counts || !effective)) return LC3_NULL_ERROR;
    for (int s = 0; s < n_streams; s++) effective[s] = lc3d_dec_count_clamp(counts[s], n_frames);
    return LC3_OK;
}
/* ---- the frame probe's host side (include/lc3plus_batch.h "Frame probe"; lc3_probe_shim.h): what needs the decoder's tables; the call itself is lc3_packet.c's ---- */
const char* lc3plus_reject_name(int code)
{
    static const char* const names[LC3P_REJ_COUNT] = {"none", "bandwidth", "lastnz", "sns_index_25", "sns_index_24", "tns_order", "tns_reader", "tns_symbol",
                                                      "overlap", "spec_symbol", "escape_14", "nres"};
    return code >= 0 && code < LC3P_REJ_COUNT ? names[code] : "";
}
/* the SIDE depth of the probe on the host: the item rule and lc3p_side, the text the kernels run */
LC3_Error lc3plus_frame_info_side(int samplerate, int channels, float frame_ms, int hrmode, const uint8_t* frame, int num_bytes, int32_t* info)
{
    if (!info || (!frame && num_bytes > 0)) return LC3_NULL_ERROR;
    geom_t g; lc3d_dchan* tab = NULL; int tab_n = 0;
    LC3_Error e = dec_hook_table(samplerate, channels, frame_ms, hrmode, &g, &tab, &tab_n);
    if (e) return e;
    const int cls = lc3p_item_class(num_bytes, 0, num_bytes > 0 ? num_bytes : 0, num_bytes > 0 ? num_bytes : 1, tab, tab_n, channels);
    free(tab);
    memset(info, 0, sizeof(int32_t) * LC3P_WORDS * (size_t)channels);
    int refused = 0;
    for (int ch = 0; ch < channels; ch++) {
        int32_t* r = info + (size_t)ch * LC3P_WORDS;
        if (cls != LC3D_FRAME_GOOD) { r[LC3P_STATUS] = LC3P_ST_CONCEALED | (cls == LC3D_FRAME_LOST ? LC3P_ST_LOST : LC3P_ST_INVALID); continue; }
        const int nb = lc3p_chan_bytes(num_bytes, channels, ch);
        r[LC3P_NBYTES] = nb;
        if (refused) { r[LC3P_STATUS] = LC3P_ST_CONCEALED | LC3P_ST_SKIPPED; continue; }
        const uint8_t* end = frame + lc3p_chan_off(num_bytes, ch) + nb;
        uint32_t v[3] = {0, 0, 0};
        for (int j = 0; j < LC3P_TAIL_BYTES; j++) v[j >> 2] |= (uint32_t)end[-1 - j] << (8 * (j & 3));
        int Q = 0;
        r[LC3P_REASON] = lc3p_side(v[0], v[1], v[2], g.fs_idx, g.bw_bits, g.ylen, g.dms, r, &Q);
        if (r[LC3P_REASON]) { r[LC3P_STATUS] = LC3P_ST_CONCEALED; refused = 1; }
    }
    return LC3_OK;
}

/* ---- single-stream drop-in API (R/lc3.h:318-406) ---- */
struct LC3_Dec {
    int channels, samplerate, plc_mode; float frame_ms;
    geom_t g;
    int last_size[MAX_CH];           /* R/setup_dec_lc3.h last_size: bytes of the channel's last good frame */
    lc3d_dchan ch[MAX_CH];
    lc3plus_dec_batch* batch;        /* batch of one stream, created lazily at the first decode */
    uint8_t* stage_in; void* stage_pcm;
    unsigned magic;
};
#define DEC_MAGIC 0x4C433344u

int lc3_dec_get_size(int samplerate, int channels)
{
    if (!lc3_samplerate_supported(samplerate) || !lc3_channels_supported(channels)) return 0;
    return (int)sizeof(struct LC3_Dec);
}

static void dec_drop_device(LC3_Dec* d)
{
    if (d->batch) { lc3plus_dec_batch_destroy(d->batch); d->batch = NULL; }
    free(d->stage_in); free(d->stage_pcm); d->stage_in = NULL; d->stage_pcm = NULL;
}

LC3_Error lc3_dec_init(LC3_Dec* d, int samplerate, int channels, LC3_PlcMode plc_mode)
{
    if (d == NULL) return LC3_NULL_ERROR;
    if (!lc3_samplerate_supported(samplerate)) return LC3_SAMPLERATE_ERROR;
    if (!lc3_channels_supported(channels)) return LC3_CHANNELS_ERROR;
    if ((int)plc_mode != LC3_PLC_STANDARD) return LC3_PLCMODE_ERROR;      /* R/lc3.c:64-72 */
    memset(d, 0, sizeof *d);
    d->magic = DEC_MAGIC; d->channels = channels; d->samplerate = samplerate; d->frame_ms = 10; d->plc_mode = (int)plc_mode;
    geom_init(&d->g, samplerate, channels);
    geom_update_ex(&d->g, 1);
    return LC3_OK;
}

/* Changing the frame size or hrmode restarts the stream with fresh memories (the reference keeps the old buffers,
 * R/setup_dec_lc3.c:73-199, whose contents belong to the other frame size; no caller in the reference does this mid-stream) */
LC3_Error lc3_dec_set_frame_ms(LC3_Dec* d, float frame_ms)
{
    if (d == NULL) return LC3_NULL_ERROR;
    { int k = (int)ceil(frame_ms * 10); if (k != 25 && k != 50 && k != 100) return LC3_FRAMEMS_ERROR; }
    d->g.dms = (int)(frame_ms * 10); d->g.frame_ms = frame_ms; d->frame_ms = frame_ms;
    geom_update_ex(&d->g, 1);
    dec_drop_device(d);
    memset(d->last_size, 0, sizeof d->last_size); memset(d->ch, 0, sizeof d->ch);
    return LC3_OK;
}

LC3_Error lc3_dec_set_hrmode(LC3_Dec* d, int hrmode)
{
    if (d == NULL) return LC3_NULL_ERROR;
    if (d->g.fs_idx < 4 && hrmode != 0) return LC3_SAMPLERATE_ERROR;
    if (d->g.fs_idx == 5 && hrmode == 0) return LC3_HRMODE_ERROR;
    d->g.hrmode = hrmode > 0;
    geom_update_ex(&d->g, 1);
    dec_drop_device(d);
    memset(d->last_size, 0, sizeof d->last_size); memset(d->ch, 0, sizeof d->ch);
    return LC3_OK;
}

int lc3_dec_get_output_samples(const LC3_Dec* d) { return d ? d->g.N : 0; }
int lc3_dec_get_delay(const LC3_Dec* d) { return d ? d->g.N - 2 * d->g.la : 0; }

LC3_Error lc3_dec_fl(LC3_Dec* d, void* input_bytes, int num_bytes, void** output_samples, int bps, int bfi_ext)
{
    if (!d || !input_bytes || !output_samples) return LC3_NULL_ERROR;
    for (int c = 0; c < d->channels; c++) if (output_samples[c] == NULL) return LC3_NULL_ERROR;
    if (bps != 16 && bps != 24 && bps != 32) return LC3_ERROR;
    if (num_bytes < 0 || num_bytes > LC3_MAX_BYTES) return LC3_NUMBYTES_ERROR;
    const int N = d->g.N, C = d->channels;
    if (!d->batch) {
        LC3_Error err = lc3plus_dec_batch_create(&d->batch, 1, d->g.fs_in, C, d->g.frame_ms, d->g.hrmode, NULL, -1);
        if (err) return err;
        d->stage_in = (uint8_t*)malloc(LC3_MAX_BYTES);
        d->stage_pcm = malloc(sizeof(int32_t) * C * LC3D_MAX_N);
        if (!d->stage_in || !d->stage_pcm) { dec_drop_device(d); return LC3_ERROR; }
    }
    int bfi = bfi_ext;
    if (bfi == 0) bfi = !num_bytes;                                        /* R/dec_lc3_fl.c:140-143 */
    if (bfi != 1) {
        /* R/dec_lc3_fl.c:146-155.  (The reference skips the update of a later channel when an earlier channel of the
         * SAME frame turns out corrupt; that needs the decode result and is not reproduced: INTEGRATION.md.) */
        int changed = 0, off = 0;
        lc3d_dchan tmp[MAX_CH];
        memcpy(tmp, d->ch, sizeof tmp);
        for (int c = 0; c < C; c++) {
            const int nb2 = num_bytes / C + (c < (num_bytes % C));
            if (nb2 != d->last_size[c]) {
                LC3_Error e = derive_dchan(&d->g, nb2, &tmp[c]);
                if (e) return e;
                changed = 1;
            }
            tmp[c].in_off = off; off += tmp[c].nbytes;
        }
        if (changed || memcmp(tmp, d->ch, sizeof tmp)) {
            memcpy(d->ch, tmp, sizeof tmp);
            for (int c = 0; c < C; c++) d->last_size[c] = d->ch[c].nbytes;
            memcpy(d->batch->chans, d->ch, sizeof(lc3d_dchan) * C);
            if (lc3hip_dec_upload_chans(d->batch->dev, d->ch, 0, C)) return LC3_ERROR;
        }
    }
    const int stride = IMAX(num_bytes, lc3plus_dec_batch_num_bytes(d->batch, 0));
    memset(d->stage_in, 0, LC3_MAX_BYTES);
    memcpy(d->stage_in, input_bytes, num_bytes);
    uint8_t flag = (uint8_t)(bfi == 1), status = 0;
    LC3_Error err = lc3plus_dec_batch_decode(d->batch, d->stage_in, 0, IMAX(stride, 1), &flag, 1, d->stage_pcm, 0, bps, &status, NULL, 1);
    if (err) return err;
    const size_t ss = bps == 16 ? 2 : 4;
    for (int c = 0; c < C; c++) memcpy(output_samples[c], (char*)d->stage_pcm + ss * c * N, ss * N);
    return status ? LC3_DECODE_ERROR : LC3_OK;
}
LC3_Error lc3_dec16(LC3_Dec* d, void* in, int nb, int16_t** out, int bfi_ext) { return lc3_dec_fl(d, in, nb, (void**)out, 16, bfi_ext); }
LC3_Error lc3_dec24(LC3_Dec* d, void* in, int nb, int32_t** out, int bfi_ext) { return lc3_dec_fl(d, in, nb, (void**)out, 24, bfi_ext); }
LC3_Error lc3_dec32(LC3_Dec* d, void* in, int nb, int32_t** out, int bfi_ext) { return lc3_dec_fl(d, in, nb, (void**)out, 32, bfi_ext); }

LC3_Error lc3_free_decoder_structs(LC3_Dec* d)
{
    if (!d) return LC3_NULL_ERROR;
    if (d->magic == DEC_MAGIC) dec_drop_device(d);
    return LC3_OK;
}
LC3_Error lc3_dec_free_memory(LC3_Dec* d)
{
    if (!d) return LC3_NULL_ERROR;
    lc3_free_decoder_structs(d);
    free(d);
    return LC3_OK;
}

/* ------------------------------------------------------------------------------------------------ */
/* sharded batches (include/lc3plus_batch.h): N ordinary batches, each with a contiguous block of the  */
/* streams on a device of its own, driven by one call.  Streams never exchange anything, so a sharded   */
/* call is the per-batch call of every shard on its slice of the arguments.                             */
/* ------------------------------------------------------------------------------------------------ */
LC3_Error lc3plus_shard_block(int n_streams, int n_shards, int shard, int* first, int* count)
{
    if (!first || !count) return LC3_NULL_ERROR;
    if (n_streams < 0 || n_shards <= 0 || shard < 0 || shard >= n_shards) return LC3_ERROR;
    const int base = n_streams / n_shards, rem = n_streams % n_shards;
    *first = shard * base + IMIN(shard, rem);
    *count = base + (shard < rem);
    return LC3_OK;
}
/* the owner of a stream under that rule */
static void shard_owner(int n_streams, int n_shards, int stream, int* shard, int* local)
{
    const int base = n_streams / n_shards, rem = n_streams % n_shards, cut = rem * (base + 1);
    const int k = stream < cut ? stream / (base + 1) : rem + (stream - cut) / IMAX(base, 1);
    *shard = k; *local = stream - (k * base + IMIN(k, rem));
}
static LC3_Error shard_devices_check(int n_streams, const int* devices, int n_devices)
{
    if (!devices) return LC3_NULL_ERROR;
    if (n_devices <= 0) return LC3_ERROR;
    for (int i = 0; i < n_devices; i++) if (devices[i] < 0) return LC3_ERROR;
    return n_streams > 0 && n_devices > n_streams ? LC3_ERROR : LC3_OK;
}

/* One worker thread per shard, alive from create to destroy.  run() hands every worker the same job function and returns when all have finished it; a
 * worker calls fn(owner, its shard).  One mutex guards gen / pending / quit; what a job reads was written before run() took it, what it writes is read
 * after run() has seen pending reach 0 under it. */
typedef struct shard_pool shard_pool;
typedef struct { shard_pool* pool; int shard; } shard_worker;
struct shard_pool {
    pthread_mutex_t mu; pthread_cond_t go, done;
    int n, started, gen, pending, quit;
    pthread_t* th; shard_worker* w;
    void (*fn)(void* owner, int shard); void* owner;
};
static void* shard_worker_main(void* arg)
{
    shard_worker* w = (shard_worker*)arg;
    shard_pool* p = w->pool;
    int seen = 0;
    pthread_mutex_lock(&p->mu);
    for (;;) {
        while (p->gen == seen && !p->quit) pthread_cond_wait(&p->go, &p->mu);
        if (p->quit) break;
        seen = p->gen;
        void (*fn)(void*, int) = p->fn; void* owner = p->owner;
        pthread_mutex_unlock(&p->mu);
        fn(owner, w->shard);
        pthread_mutex_lock(&p->mu);
        if (--p->pending == 0) pthread_cond_signal(&p->done);
    }
    pthread_mutex_unlock(&p->mu);
    return NULL;
}
static void shard_pool_stop(shard_pool* p)
{
    pthread_mutex_lock(&p->mu); p->quit = 1; pthread_cond_broadcast(&p->go); pthread_mutex_unlock(&p->mu);
    for (int i = 0; i < p->started; i++) pthread_join(p->th[i], NULL);
    pthread_cond_destroy(&p->go); pthread_cond_destroy(&p->done); pthread_mutex_destroy(&p->mu);
    free(p->th); free(p->w);
}
static int shard_pool_start(shard_pool* p, int n, void* owner)
{
    memset(p, 0, sizeof *p);
    p->n = n; p->owner = owner;
    p->th = (pthread_t*)calloc((size_t)n, sizeof(pthread_t)); p->w = (shard_worker*)calloc((size_t)n, sizeof(shard_worker));
    if (!p->th || !p->w) { free(p->th); free(p->w); return 1; }
    pthread_mutex_init(&p->mu, NULL); pthread_cond_init(&p->go, NULL); pthread_cond_init(&p->done, NULL);
    for (int i = 0; i < n; i++) {
        p->w[i].pool = p; p->w[i].shard = i;
        if (pthread_create(&p->th[i], NULL, shard_worker_main, &p->w[i])) { shard_pool_stop(p); return 1; }
        p->started++;
    }
    return 0;
}
static void shard_pool_run(shard_pool* p, void (*fn)(void*, int))
{
    pthread_mutex_lock(&p->mu);
    p->fn = fn; p->pending = p->n; p->gen++;
    pthread_cond_broadcast(&p->go);
    while (p->pending) pthread_cond_wait(&p->done, &p->mu);
    pthread_mutex_unlock(&p->mu);
}
/* LC3_OK if every shard returned it, otherwise the first other code in shard order */
static LC3_Error shard_result(const LC3_Error* res, int n)
{
    for (int i = 0; i < n; i++) if (res[i] != LC3_OK) return res[i];
    return LC3_OK;
}

/* What a sharded batch of either kind is made of: the split, the shards' batches (lc3plus_batch* of an encoder, lc3plus_dec_batch* of a decoder), the result of
 * every shard's last call and the workers.  lc3plus_sharded and lc3plus_dec_sharded hold one, what they answer without asking a shard, and the arguments of the
 * host-pointer call their workers are running.  The helpers take the set of a handle or NULL for a NULL handle (SET), so that an entry point is one line that
 * says what it returns where there is no such handle, shard or stream. */
typedef struct {
    int n_streams, n_shards, decoder;
    void** sh; int* first; int* count; int* dev; LC3_Error* res;
    shard_pool pool;
} shard_set;
#define SET(s) ((s) ? &(s)->set : NULL)

/* destroys the first `created` shards and frees the arrays (not the workers: shard_pool_stop) */
static void shard_set_close(shard_set* s, int created)
{
    for (int k = 0; k < created; k++) { if (s->decoder) lc3plus_dec_batch_destroy((lc3plus_dec_batch*)s->sh[k]); else lc3plus_enc_batch_destroy((lc3plus_batch*)s->sh[k]); }
    free(s->sh); free(s->first); free(s->count); free(s->dev); free(s->res);
}
/* The arrays, every shard's batch - created on its device with its block of cfg (the streams' bitrates or frame sizes; NULL: none) - and the workers, which
 * hand `owner` to their jobs.  Returns the first error, with nothing left behind. */
static LC3_Error shard_set_open(shard_set* s, void* owner, int decoder, int n_streams, int samplerate, int channels, float frame_ms, int hrmode, const int* cfg,
                                const int* devices, int n_devices)
{
    s->n_streams = n_streams; s->n_shards = n_devices; s->decoder = decoder;
    s->sh = (void**)calloc((size_t)n_devices, sizeof *s->sh);
    s->first = (int*)calloc((size_t)n_devices, sizeof(int)); s->count = (int*)calloc((size_t)n_devices, sizeof(int));
    s->dev = (int*)calloc((size_t)n_devices, sizeof(int)); s->res = (LC3_Error*)calloc((size_t)n_devices, sizeof(LC3_Error));
    if (!s->sh || !s->first || !s->count || !s->dev || !s->res) { shard_set_close(s, 0); return LC3_ERROR; }
    for (int k = 0; k < n_devices; k++) {
        lc3plus_shard_block(n_streams, n_devices, k, &s->first[k], &s->count[k]);
        s->dev[k] = devices[k];
        const int* c = cfg ? cfg + s->first[k] : NULL;
        lc3plus_batch* eb = NULL; lc3plus_dec_batch* db = NULL;
        const LC3_Error e = decoder ? lc3plus_dec_batch_create(&db, s->count[k], samplerate, channels, frame_ms, hrmode, c, devices[k])
                                    : lc3plus_enc_batch_create(&eb, s->count[k], samplerate, channels, frame_ms, hrmode, c, devices[k]);
        if (e) { shard_set_close(s, k); return e; }
        s->sh[k] = decoder ? (void*)db : (void*)eb;
    }
    if (shard_pool_start(&s->pool, n_devices, owner)) { shard_set_close(s, n_devices); return LC3_ERROR; }
    return LC3_OK;
}
static int shard_set_shards(const shard_set* s) { return s ? s->n_shards : 0; }
static void* shard_set_shard(const shard_set* s, int shard) { return s && shard >= 0 && shard < s->n_shards ? s->sh[shard] : NULL; }
static int shard_set_device(const shard_set* s, int shard) { return s && shard >= 0 && shard < s->n_shards ? s->dev[shard] : -1; }
static LC3_Error shard_set_owner(const shard_set* s, int stream, int* shard, int* local)
{
    if (!s || !shard || !local) return LC3_NULL_ERROR;
    if (stream < 0 || stream >= s->n_streams) return LC3_ERROR;
    shard_owner(s->n_streams, s->n_shards, stream, shard, local);
    return LC3_OK;
}
/* the batch that owns a global stream and the stream's index in it, NULL where there is none */
static void* shard_set_at(const shard_set* s, int stream, int* local)
{
    int k = 0;
    return shard_set_owner(s, stream, &k, local) ? NULL : s->sh[k];
}
/* The shards' states one after the other: [channel-stream][state words] over all the streams, which is the state of an unsharded batch of n_streams.  One walk
 * over the blocks: their sizes summed, or every shard handed its block to fill (set = 0) or to take (set = 1). */
static size_t shard_state_size(const shard_set* s, int k)
{
    return s->decoder ? lc3plus_dec_batch_state_size((lc3plus_dec_batch*)s->sh[k]) : lc3plus_enc_batch_state_size((lc3plus_batch*)s->sh[k]);
}
static size_t shard_set_state_size(const shard_set* s)
{
    size_t n = 0;
    if (s) for (int k = 0; k < s->n_shards; k++) n += shard_state_size(s, k);
    return n;
}
static LC3_Error shard_set_state(shard_set* s, void* state, size_t size, int set)
{
    if (!s || !state) return LC3_NULL_ERROR;
    if (size != shard_set_state_size(s)) return LC3_ERROR;
    uint8_t* p = (uint8_t*)state;
    for (int k = 0; k < s->n_shards; k++) {
        const size_t n = shard_state_size(s, k);
        if (s->decoder) s->res[k] = set ? lc3plus_dec_batch_set_state((lc3plus_dec_batch*)s->sh[k], p, n) : lc3plus_dec_batch_get_state((lc3plus_dec_batch*)s->sh[k], p, n);
        else s->res[k] = set ? lc3plus_enc_batch_set_state((lc3plus_batch*)s->sh[k], p, n) : lc3plus_enc_batch_get_state((lc3plus_batch*)s->sh[k], p, n);
        p += n;
    }
    return shard_result(s->res, s->n_shards);
}
/* The PCM of a host-pointer call from stream `first` on: in all three layouts the stream index is the outermost one, so the slice is an offset (none where the
 * shard's call refuses the format or the frame count anyway) */
static char* shard_pcm(const char* pcm, int fmt, int channels, int n_frames, int samples, int first)
{
    const int64_t po = pcm && n_frames > 0 && lc3d_pcm_format_ok(fmt) ? lc3plus_pcm_offset(fmt, channels, n_frames, samples, first, 0, 0, 0) : 0;
    return pcm ? (char*)pcm + (size_t)lc3d_pcm_elem_bytes(fmt) * (size_t)po : NULL;
}

/* ---- encoders ---- */
struct lc3plus_sharded {
    shard_set set; int channels, N;
    /* the arguments of the host-pointer call the workers are running */
    struct { const char* pcm; int fmt; const int* bw; const int* br; int T; uint8_t* out; int stride; int* nb; } a;
};
#define ENC_SHARD(s, k) ((lc3plus_batch*)(s)->set.sh[k])

LC3_Error lc3plus_enc_sharded_create(lc3plus_sharded** out, int n_streams, int samplerate, int channels, float frame_ms, int hrmode, const int* bitrates,
                                     const int* devices, int n_devices)
{
    if (!out || !bitrates) return LC3_NULL_ERROR;
    *out = NULL;
    LC3_Error e = shard_devices_check(n_streams, devices, n_devices);
    if (e) return e;
    geom_t g;
    e = enc_batch_geometry(&g, n_streams, samplerate, channels, frame_ms, hrmode);
    if (e) return e;
    for (int i = 0; i < n_streams; i++) { lc3d_chan tmp[MAX_CH]; e = derive_bitrate(&g, bitrates[i], tmp); if (e) return e; }      /* before any device is touched */
    lc3plus_sharded* s = (lc3plus_sharded*)calloc(1, sizeof *s);
    if (!s) return LC3_ERROR;
    s->channels = channels; s->N = g.N;
    e = shard_set_open(&s->set, s, 0, n_streams, samplerate, channels, frame_ms, hrmode, bitrates, devices, n_devices);
    if (e) { free(s); return e; }
    *out = s;
    return LC3_OK;
}
LC3_Error lc3plus_enc_sharded_destroy(lc3plus_sharded* s)
{
    if (!s) return LC3_NULL_ERROR;
    shard_pool_stop(&s->set.pool);
    shard_set_close(&s->set, s->set.n_shards);
    free(s);
    return LC3_OK;
}
int lc3plus_enc_sharded_shards(const lc3plus_sharded* s) { return shard_set_shards(SET(s)); }
lc3plus_batch* lc3plus_enc_sharded_shard(lc3plus_sharded* s, int shard) { return (lc3plus_batch*)shard_set_shard(SET(s), shard); }
int lc3plus_enc_sharded_device(const lc3plus_sharded* s, int shard) { return shard_set_device(SET(s), shard); }
LC3_Error lc3plus_enc_sharded_owner(const lc3plus_sharded* s, int stream, int* shard, int* local) { return shard_set_owner(SET(s), stream, shard, local); }
int lc3plus_enc_sharded_input_samples(const lc3plus_sharded* s) { return s ? s->N : 0; }
int lc3plus_enc_sharded_num_bytes(const lc3plus_sharded* s, int stream)
{
    int l = 0; lc3plus_batch* b = (lc3plus_batch*)shard_set_at(SET(s), stream, &l);
    return b ? lc3plus_enc_batch_num_bytes(b, l) : 0;
}
int lc3plus_enc_sharded_stride(const lc3plus_sharded* s)
{
    int m = 0;
    if (!s) return 0;
    for (int k = 0; k < s->set.n_shards; k++) { const int v = lc3plus_enc_batch_stride(ENC_SHARD(s, k)); if (v <= 0) return 0; m = IMAX(m, v); }
    return m;
}
LC3_Error lc3plus_enc_sharded_set_bitrate(lc3plus_sharded* s, int stream, int bitrate)
{
    if (!s) return LC3_NULL_ERROR;
    int l = 0; lc3plus_batch* b = (lc3plus_batch*)shard_set_at(&s->set, stream, &l);
    return b ? lc3plus_enc_batch_set_bitrate(b, l, bitrate) : LC3_ERROR;
}
LC3_Error lc3plus_enc_sharded_set_bandwidth(lc3plus_sharded* s, int stream, int bandwidth)
{
    if (!s) return LC3_NULL_ERROR;
    int l = 0; lc3plus_batch* b = (lc3plus_batch*)shard_set_at(&s->set, stream, &l);
    return b ? lc3plus_enc_batch_set_bandwidth(b, l, bandwidth) : LC3_ERROR;
}
int lc3plus_enc_sharded_bandwidth(const lc3plus_sharded* s, int stream)
{
    int l = 0; lc3plus_batch* b = (lc3plus_batch*)shard_set_at(SET(s), stream, &l);
    return b ? lc3plus_enc_batch_bandwidth(b, l) : -1;
}

/* shard k's call of the host-pointer encode: the call an unsharded batch would be given for the same arguments, on the shard's slice of every array */
static LC3_Error enc_shard_call(lc3plus_sharded* s, int k)
{
    const size_t f = (size_t)s->set.first[k], row = f * (size_t)(s->a.T > 0 ? s->a.T : 0);
    const char* pcm = shard_pcm(s->a.pcm, s->a.fmt, s->channels, s->a.T, s->N, (int)f);
    uint8_t* out = s->a.out ? s->a.out + row * (size_t)(s->a.stride > 0 ? s->a.stride : 0) : NULL;
    const int* br = s->a.br ? s->a.br + row : NULL;
    int* nb = s->a.nb ? s->a.nb + row : NULL;
    lc3plus_batch* b = ENC_SHARD(s, k);
    if (s->a.bw) return batch_encode_bandwidths(b, pcm, 0, s->a.fmt, s->a.bw + row, br, s->a.T, out, s->a.stride, 0, nb, NULL, 1);
    if (s->a.br) return batch_encode_bitrates(b, pcm, 0, s->a.fmt, br, s->a.T, out, s->a.stride, 0, nb, NULL, 1, NULL);
    const LC3_Error e = batch_encode(b, pcm, 0, s->a.fmt, s->a.T, out, s->a.stride, 0, NULL, 1, NULL);
    if (!e && nb && !b->dry) for (size_t i = 0; i < (size_t)s->set.count[k] * s->a.T; i++) nb[i] = lc3plus_enc_batch_num_bytes(b, (int)(i / s->a.T));
    return e;
}
static void enc_shard_job(void* owner, int k) { lc3plus_sharded* s = (lc3plus_sharded*)owner; s->set.res[k] = enc_shard_call(s, k); }
/* Every check of the call on every shard, on the calling thread, nothing run: step by step over all shards, so that the code is the one an unsharded batch
 * gives (DRY_*).  LC3_OK and LC3_BW_WARNING let the call go on. */
static LC3_Error enc_sharded_check(lc3plus_sharded* s)
{
    LC3_Error res = LC3_OK;
    for (int step = s->a.bw ? DRY_BW : s->a.br ? DRY_RATES : DRY_ALL; step <= DRY_ALL && (res == LC3_OK || res == LC3_BW_WARNING); step++) {
        if (step == DRY_RATES && !s->a.br) continue;
        for (int k = 0; k < s->set.n_shards && (res == LC3_OK || res == LC3_BW_WARNING); k++) {
            ENC_SHARD(s, k)->dry = step;
            const LC3_Error e = enc_shard_call(s, k);
            ENC_SHARD(s, k)->dry = 0;
            if (e) res = e;
        }
    }
    return res;
}
LC3_Error lc3plus_enc_sharded_encode(lc3plus_sharded* s, const void* pcm, int bitdepth, const int* bandwidths, const int* bitrates, int n_frames, void* out,
                                     int out_stride, int* num_bytes)
{
    if (!s) return LC3_NULL_ERROR;
    s->a.pcm = (const char*)pcm; s->a.fmt = bitdepth; s->a.bw = bandwidths; s->a.br = bitrates; s->a.T = n_frames; s->a.out = (uint8_t*)out;
    s->a.stride = out_stride; s->a.nb = num_bytes;
    const LC3_Error e = enc_sharded_check(s);
    if (e != LC3_OK && e != LC3_BW_WARNING) return e;
    shard_pool_run(&s->set.pool, enc_shard_job);
    return shard_result(s->set.res, s->set.n_shards);
}
LC3_Error lc3plus_enc_sharded_encode_device(lc3plus_sharded* s, const void* const* pcm, int bitdepth, int n_frames, void* const* out, int out_stride,
                                            void* const* hip_streams, int sync)
{
    if (!s || !pcm || !out) return LC3_NULL_ERROR;
    for (int k = 0; k < s->set.n_shards; k++) {
        ENC_SHARD(s, k)->dry = DRY_ALL;
        const LC3_Error e = batch_encode(ENC_SHARD(s, k), pcm[k], 1, bitdepth, n_frames, out[k], out_stride, 1, NULL, 0, NULL);
        ENC_SHARD(s, k)->dry = 0;
        if (e) return e;
    }
    /* every shard's call is queued before any is waited for */
    for (int k = 0; k < s->set.n_shards; k++)
        s->set.res[k] = batch_encode(ENC_SHARD(s, k), pcm[k], 1, bitdepth, n_frames, out[k], out_stride, 1, hip_streams ? hip_streams[k] : NULL, 0, NULL);
    if (sync) for (int k = 0; k < s->set.n_shards; k++) if (lc3hip_wait(ENC_SHARD(s, k)->dev) && !s->set.res[k]) s->set.res[k] = LC3_ERROR;
    return shard_result(s->set.res, s->set.n_shards);
}
size_t lc3plus_enc_sharded_state_size(const lc3plus_sharded* s) { return shard_set_state_size(SET(s)); }
LC3_Error lc3plus_enc_sharded_get_state(lc3plus_sharded* s, void* state, size_t size) { return shard_set_state(SET(s), state, size, 0); }
LC3_Error lc3plus_enc_sharded_set_state(lc3plus_sharded* s, const void* state, size_t size) { return shard_set_state(SET(s), (void*)state, size, 1); }
float lc3plus_enc_sharded_last_kernel_ms(lc3plus_sharded* s, int shard) { return lc3plus_enc_batch_last_kernel_ms((lc3plus_batch*)shard_set_shard(SET(s), shard)); }

/* ---- decoders ---- */
struct lc3plus_dec_sharded {
    shard_set set; int channels, N, delay;
    struct { const uint8_t* frames; int in_stride; const int* nb; const uint8_t* bfi; int T; char* pcm; int fmt; uint8_t* status; } a;
};
#define DEC_SHARD(s, k) ((lc3plus_dec_batch*)(s)->set.sh[k])

LC3_Error lc3plus_dec_sharded_create(lc3plus_dec_sharded** out, int n_streams, int samplerate, int channels, float frame_ms, int hrmode, const int* num_bytes,
                                     const int* devices, int n_devices)
{
    if (!out) return LC3_NULL_ERROR;
    *out = NULL;
    LC3_Error e = shard_devices_check(n_streams, devices, n_devices);
    if (e) return e;
    geom_t g;
    e = dec_batch_geometry(&g, n_streams, samplerate, channels, frame_ms, hrmode);
    if (e) return e;
    if (num_bytes) for (int i = 0; i < n_streams; i++) { lc3d_dchan tmp[MAX_CH]; memset(tmp, 0, sizeof tmp); e = derive_dstream(&g, num_bytes[i], tmp); if (e) return e; }
    lc3plus_dec_sharded* s = (lc3plus_dec_sharded*)calloc(1, sizeof *s);
    if (!s) return LC3_ERROR;
    s->channels = channels; s->N = g.N; s->delay = g.N - 2 * g.la;
    e = shard_set_open(&s->set, s, 1, n_streams, samplerate, channels, frame_ms, hrmode, num_bytes, devices, n_devices);
    if (e) { free(s); return e; }
    *out = s;
    return LC3_OK;
}
LC3_Error lc3plus_dec_sharded_destroy(lc3plus_dec_sharded* s)
{
    if (!s) return LC3_NULL_ERROR;
    shard_pool_stop(&s->set.pool);
    shard_set_close(&s->set, s->set.n_shards);
    free(s);
    return LC3_OK;
}
int lc3plus_dec_sharded_shards(const lc3plus_dec_sharded* s) { return shard_set_shards(SET(s)); }
lc3plus_dec_batch* lc3plus_dec_sharded_shard(lc3plus_dec_sharded* s, int shard) { return (lc3plus_dec_batch*)shard_set_shard(SET(s), shard); }
int lc3plus_dec_sharded_device(const lc3plus_dec_sharded* s, int shard) { return shard_set_device(SET(s), shard); }
LC3_Error lc3plus_dec_sharded_owner(const lc3plus_dec_sharded* s, int stream, int* shard, int* local) { return shard_set_owner(SET(s), stream, shard, local); }
int lc3plus_dec_sharded_output_samples(const lc3plus_dec_sharded* s) { return s ? s->N : 0; }
int lc3plus_dec_sharded_delay(const lc3plus_dec_sharded* s) { return s ? s->delay : 0; }
int lc3plus_dec_sharded_num_bytes(const lc3plus_dec_sharded* s, int stream)
{
    int l = 0; lc3plus_dec_batch* b = (lc3plus_dec_batch*)shard_set_at(SET(s), stream, &l);
    return b ? lc3plus_dec_batch_num_bytes(b, l) : 0;
}
LC3_Error lc3plus_dec_sharded_set_num_bytes(lc3plus_dec_sharded* s, int stream, int num_bytes)
{
    if (!s) return LC3_NULL_ERROR;
    int l = 0; lc3plus_dec_batch* b = (lc3plus_dec_batch*)shard_set_at(&s->set, stream, &l);
    return b ? lc3plus_dec_batch_set_num_bytes(b, l, num_bytes) : LC3_ERROR;
}
static LC3_Error dec_shard_call(lc3plus_dec_sharded* s, int k)
{
    const size_t f = (size_t)s->set.first[k], row = f * (size_t)(s->a.T > 0 ? s->a.T : 0);
    char* pcm = shard_pcm(s->a.pcm, s->a.fmt, s->channels, s->a.T, s->N, (int)f);
    const uint8_t* frames = s->a.frames ? s->a.frames + row * (size_t)(s->a.in_stride > 0 ? s->a.in_stride : 0) : NULL;
    const uint8_t* bfi = s->a.bfi ? s->a.bfi + row : NULL;
    uint8_t* status = s->a.status ? s->a.status + row : NULL;
    if (s->a.nb) return lc3plus_dec_batch_decode_sizes(DEC_SHARD(s, k), frames, 0, s->a.in_stride, s->a.nb + row, bfi, s->a.T, pcm, 0, s->a.fmt, status, NULL, 1);
    return dec_batch_decode(DEC_SHARD(s, k), frames, 0, s->a.in_stride, bfi, s->a.T, pcm, 0, s->a.fmt, status, NULL, 1, NULL);
}
static void dec_shard_job(void* owner, int k) { lc3plus_dec_sharded* s = (lc3plus_dec_sharded*)owner; s->set.res[k] = dec_shard_call(s, k); }
LC3_Error lc3plus_dec_sharded_decode(lc3plus_dec_sharded* s, const void* frames, int in_stride, const int* num_bytes, const uint8_t* bfi, int n_frames, void* pcm,
                                     int bps, uint8_t* status)
{
    if (!s) return LC3_NULL_ERROR;
    s->a.frames = (const uint8_t*)frames; s->a.in_stride = in_stride; s->a.nb = num_bytes; s->a.bfi = bfi; s->a.T = n_frames; s->a.pcm = (char*)pcm;
    s->a.fmt = bps; s->a.status = status;
    /* every check on every shard first, nothing run: shards are blocks of streams in order, and the checks walk the streams in order, so the first refusal
     * is the unsharded batch's */
    for (int k = 0; k < s->set.n_shards; k++) {
        DEC_SHARD(s, k)->dry = DRY_ALL;
        const LC3_Error e = dec_shard_call(s, k);
        DEC_SHARD(s, k)->dry = 0;
        if (e) return e;
    }
    shard_pool_run(&s->set.pool, dec_shard_job);
    return shard_result(s->set.res, s->set.n_shards);
}
LC3_Error lc3plus_dec_sharded_decode_device(lc3plus_dec_sharded* s, const void* const* frames, int in_stride, int n_frames, void* const* pcm, int bps,
                                            void* const* hip_streams, int sync)
{
    if (!s || !frames || !pcm) return LC3_NULL_ERROR;
    for (int k = 0; k < s->set.n_shards; k++) {
        DEC_SHARD(s, k)->dry = DRY_ALL;
        const LC3_Error e = dec_batch_decode(DEC_SHARD(s, k), frames[k], 1, in_stride, NULL, n_frames, pcm[k], 1, bps, NULL, NULL, 0, NULL);
        DEC_SHARD(s, k)->dry = 0;
        if (e) return e;
    }
    for (int k = 0; k < s->set.n_shards; k++)
        s->set.res[k] = dec_batch_decode(DEC_SHARD(s, k), frames[k], 1, in_stride, NULL, n_frames, pcm[k], 1, bps, NULL, hip_streams ? hip_streams[k] : NULL, 0, NULL);
    if (sync) for (int k = 0; k < s->set.n_shards; k++) if (lc3hip_dec_wait(DEC_SHARD(s, k)->dev) && !s->set.res[k]) s->set.res[k] = LC3_ERROR;
    return shard_result(s->set.res, s->set.n_shards);
}
size_t lc3plus_dec_sharded_state_size(const lc3plus_dec_sharded* s) { return shard_set_state_size(SET(s)); }
LC3_Error lc3plus_dec_sharded_get_state(lc3plus_dec_sharded* s, void* state, size_t size) { return shard_set_state(SET(s), state, size, 0); }
LC3_Error lc3plus_dec_sharded_set_state(lc3plus_dec_sharded* s, const void* state, size_t size) { return shard_set_state(SET(s), (void*)state, size, 1); }
float lc3plus_dec_sharded_last_kernel_ms(lc3plus_dec_sharded* s, int shard) { return lc3plus_dec_batch_last_kernel_ms((lc3plus_dec_batch*)shard_set_shard(SET(s), shard)); }
