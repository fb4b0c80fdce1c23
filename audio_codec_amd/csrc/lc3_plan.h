/* lc3_plan.h -- structures shared by the host C code (lc3_host.c) and the HIP kernels (lc3_kernels.hip).
 *
 * lc3d_plan : everything that is constant for a batch (geometry derived as in R/setup_enc_lc3.c:73-193 and
 *             the init-time tables the reference builds with libm at start-up: DCT-IV twiddles R/dct4.c:51-63,
 *             DCT-II(16) twiddles R/dct4.c:43-45, IDCT-II cosines R/sns_quantize_scf.c:30, SNS pre-emphasis
 *             R/sns_compute_scf.c:91, global-gain powers R/estimate_global_gain.c:136 / R/adjust_global_gain.c:47).
 *             Built on the host with the host libm -- exactly where the reference evaluates them -- and uploaded once.
 * lc3d_chan : per channel-stream bitrate-derived values (R/setup_enc_lc3.c:196-375).
 * State     : per channel-stream cross-frame state (R/setup_enc_lc3.h:17-62), LC3D_STATE_WORDS 32-bit words in HBM.
 */
#ifndef LC3_PLAN_H
#define LC3_PLAN_H
#include <stddef.h>
#include <stdint.h>

#define LC3D_MAX_N 960          /* largest frame length (96 kHz / 10 ms); the kernels come in two LDS layouts, see lc3_kernels.hip */
#define LC3D_PFA_STRIDE 160     /* longest prime-factor DFT (32 kHz / 10 ms: 160 = 32 x 5) */
#define LC3D_GAIN_TAB 512       /* gain index k = ind + gg_off in [-256, 255] -> tab[k + 256] */

typedef struct {
    int32_t fs, fs_idx, dms, hrmode, N, ylen, la, nbands, bw_bits, fft_len, channels;
    int32_t rs_mem_in_len, rs_stride, len12, n12, ltpf_mem_len;
    int32_t att_nblocks, att_hang, bw_cls, win_off, band_off, tilt;
    float   att_damping, sns_damping, rs_scale, frame_ms, dct4_norm;
    /* float constants the reference obtains from powf()/sqrtf() at run time with constant arguments */
    float   c_1em5_a;           /* powf(10.0,-5.0)  R/olpa.c:112 */
    float   c_1em5_b;           /* powf(10,-5)      R/ltpf_coder.c:97 */
    float   c_1em4;             /* powf(10.0,-4.0)  R/sns_compute_scf.c:101 */
    float   c_2m32, c_2m31, c_2m24, c_2p15, c_2p100;
    float   c_sqrt2;            /* sqrtf(2) */
    float   c_idct_n1, c_idct_n2;   /* R/sns_quantize_scf.c:24-25 */
    float   c_thr7_up;          /* smallest float >= (7.0)*(28.0/20.0):  (double)t < thr  <=>  t < c_thr7_up  (R/estimate_global_gain.c:106) */
    float   c_thr50_dn;         /* largest float <= (50.0)*(28.0/20.0): (double)t > thr  <=>  t > c_thr50_dn (R/estimate_global_gain.c:111) */
    int32_t pfa_nst;            /* prime-factor DFT stages (2 or 3) for N/2 in {10,20,30,40,80,120,160}; 0: N/2 = 240 or 60 use their own kernels */
    int32_t pfa_rad[3];         /* stage radices (leaf DFT lengths), in execution order */
    float   pad0;
    float   tw1[LC3D_MAX_N], tw2[LC3D_MAX_N];      /* N/2 complex (re,im) pairs each */
    float   dct2_tw[32];
    float   sns_preemph[64];
    float   gain_est[LC3D_GAIN_TAB];               /* powf(10, (k)/28.0)  (double division) */
    float   gain_adj[LC3D_GAIN_TAB];               /* powf(10, (float)k/28) (float division) */
    float   rs_taps[240];                          /* 12.8 kHz resampler low-pass, phase-major: [start][m] = lp[239 - start - m*stride] (R/resamp12k8.c:48-57) */
    double  idct_cos[256];
    /* quantiser bit estimate (R/quantize_spec.c:60-170), derived from the arithmetic-coder tables so that a 2-tuple costs three loads:
     * per context t in [0, 1024): the probability-model index of each of the four escape classes in one word; the cost of the
     * escape symbols as cumulative sums over the classes; and the bit-cost table itself behind the same base pointer */
    uint16_t q_esc[1024][4];    /* e0, e0 + e1, e0 + e1 + e2, e3   with e_j = ac_bits[ctx_lut[t + 1024 j] * 17 + 16] (3 x 20480 < 2^16) */
    uint32_t q_lut4[1024];      /* ctx_lut[t] | ctx_lut[t + 1024] << 8 | ctx_lut[t + 2048] << 16 | ctx_lut[t + 3072] << 24 */
    uint16_t q_bits[1088];      /* = lc3t_ac_bits */
    uint8_t band_of_bin[LC3D_MAX_N];
    uint8_t pfa_src[3 * LC3D_PFA_STRIDE];   /* prime-factor DFT: gather maps of up to three stages; for N/2 = 60: [0..59] = (45k+16l)%60 */
    uint8_t pfa_dst[LC3D_PFA_STRIDE];       /* scatter of the last stage; for N/2 = 60: (15k+4l)%60 */
} lc3d_plan;
#define LC3D_PLAN_HEAD_WORDS 45     /* the scalar head (up to and including pad0) that every wave copies into LDS */

typedef struct {
    int32_t nbytes, total_bits, target_bits_init, lpc_weighting, ltpf_enable, gg_off, attack_handling, reg_bits;
    int32_t out_off;            /* byte offset of this channel's payload inside the stream-frame */
    int32_t bandwidth, bw_cut_bin, bw_index;
    int32_t reset_attack;       /* set by a bitrate change that disables attack handling (R/setup_enc_lc3.c:297-308) */
    int32_t bitrate;            /* the stream's total bitrate (all channels) these values come from; no kernel reads it: the host reads it back */
    int32_t pad[2];
} lc3d_chan;

/* ---- state layout (32-bit words), parametrised by the kernel layout's MDCT-memory slot (300 standard, 600 large) ---- */
#define LC3D_MEMCAP_STD 300
#define LC3D_MEMCAP_BIG 600                       /* 96 kHz / 10 ms: N - la_zeros = 960 - 360 */
#define LC3D_LAYOUT_BIG(N, la) ((N) > 480 || (N) - (la) > LC3D_MEMCAP_STD)
#define LC3D_ST_XPREV   0                         /* MDCT / resampler memory: tail of the previous frame, right-aligned in the slot */
#define LC3D_H12_KEEP   384                       /* last 384 samples of the HP-filtered 12.8 kHz stream */
#define LC3D_H6_KEEP    194                       /* last 194 samples of the 6.4 kHz stream */
#define LC3D_ST_H12(mc)  (LC3D_ST_XPREV + (mc))
#define LC3D_ST_H6(mc)   (LC3D_ST_H12(mc) + LC3D_H12_KEEP)
#define LC3D_ST_SCAL(mc) (LC3D_ST_H6(mc) + LC3D_H6_KEEP + 2)   /* 16 float scalars (kernel fsc[0..15]) then 16 int scalars (isc[0..15]) */
#define LC3D_S_OLPA_PITCH_WORD(mc) (LC3D_ST_SCAL(mc) + 16 + 0) /* isc[I_OLPA_PITCH]: initial value 17 (R/setup_enc_lc3.c:178) */
#define LC3D_STATE_WORDS(mc) ((mc) + 660)
#define LC3D_STATE_WORDS_MAX LC3D_STATE_WORDS(LC3D_MEMCAP_BIG)

/* hand-over from the frame-parallel front of the encoder (lc3_enc_front_kernel: MDCT, band energies, bandwidth, SNS scale factors) through
 * the one-frame-per-lane vector quantiser (lc3_enc_snsvq_kernel) to the sequential kernel: per channel-frame a record of FR_WORDS words
 * and the MDCT spectrum row of N floats */
#define FR_SCF   0                       /* 16 floats: scale factors (R/sns_compute_scf.c) */
#define FR_SCFQ  16                      /* 16 floats: quantised scale factors (R/sns_quantize_scf.c) */
#define FR_IDX   32                      /* 7 ints: the SNS indices */
#define FR_BW    39                      /* int: bandwidth index (R/detect_cutoff_warped.c) */
#define FR_ATT   40                      /* attack detector (R/attack_detector.c): 4 block energies, [44..45] the filter memory after this frame, [46] the flag (lc3_enc_attack_kernel) */
#define FR_ATTM  44
#define FR_ATTFLAG 46
#define FR_LTPF  48                      /* 4 ints from lc3_enc_pitch_kernel: LTPF flag, active, pitch index, side bits (R/ltpf_coder.c:245-254) */
#define FR_TNS   52                      /* 20 ints from lc3_enc_shape_kernel: filters, orders (2), bits, coefficient indices (16) = isc[I_TNS_NF ...] (R/tns_coder.c) */
#define FR_GGMIN 72                      /* float: smallest gain index of the frame, before the offset (R/estimate_global_gain.c:72-77) */
#define FR_XZERO 73                      /* int: the shaped spectrum is all zero (:65-70) */
#define FR_BWC   74                      /* int: bandwidth index behind the bandwidth controller (R/cutoff_bandwidth.c) */
#define FR_RATE  76                      /* 4 words from lc3_enc_rate_kernel: gain index (int), gain (float), bits of the first quantisation, its lastnz */
#define FR_WORDS 80
/* spectrum row of the pipelined encoder path, per channel-frame: [0, ylen) the MDCT spectrum (lc3_enc_front_kernel), shaped and TNS-filtered in
 * place by lc3_enc_shape_kernel, which appends the ylen / 4 log energies of the gain estimate; rows are SROW words apart */
#define LC3D_SROW(ylen) (((ylen) + ((ylen) >> 2) + 15) & ~15)
/* Storage: a row is SROW / 16 chunks of 16 floats, and chunk c of row (cs, t) lies at ((cs * NCH + c) * RT + t) * 16 (RT rows per channel-stream):
 * the same chunk of consecutive frames of a stream is adjacent in memory.  The one-frame-per-lane kernels give 64 consecutive frames to the
 * 64 lanes of a wave, so each of their 64-byte-per-lane accesses is one 4 KB run; a wave that owns one frame reads 64-byte segments. */
#define LC3D_ROW_BASE(rows, cs, t, RT, srow) ((rows) + (((size_t)(cs) * ((srow) >> 4)) * (size_t)(RT) + (size_t)(t)) * 16)
#define LC3D_ROW_OFF(k, RT) (((((size_t)((k) >> 4)) * (size_t)(RT)) << 4) + (size_t)((k) & 15))

/* per channel-frame status bits of the encoder: conditions the reference only asserts on (SURVEY 5 "failure detection") */
#define LC3D_ENC_ST_BIT_BUDGET  1        /* side information + range-coder bits exceed the frame (R/ari_codec.c:777) */
#define LC3D_ENC_ST_QUANT_RANGE 2        /* a quantised line outside int16 without the high-resolution mode (R/quantize_spec.c:50) */

/* ---- decoder (lc3_dec_kernels.inc) ---- */
#define DEC_LY 864                       /* LTPF output history: ceil(228 * 48000 / 12800) + 6 = 861 */
#define DEC_LX 16                        /* LTPF input history (tilt filter length - 1 <= 10) */
typedef struct {                         /* per channel-stream decoder configuration, R/setup_dec_lc3.c:188-299 */
    int32_t nbytes, lpc_weighting, gg_off, N_red_tns, fs_red_tns, ltpf_beta_idx; float ltpf_beta; int32_t in_off;
} lc3d_dchan;

/* The per-frame rule of the per-frame-size decode calls, one (stream, frame) at a time, on the host (lc3_host.c: the checks of
 * lc3plus_dec_batch_decode_sizes, the test hooks) and on the device (lc3_dec_plan_sizes_kernel).  tab[tab_n]: the configuration per channel
 * byte count (an entry is valid where its nbytes equals its index and is not 0); a stream-frame of nb bytes is split over the channels as
 * R/dec_lc3_fl.c:148 does.  A frame is lost where bfi is 1 or its size is 0 - its size is then not looked at; a flag other than 0 / 1, and a size
 * that is negative, larger than in_stride or outside the table for any channel of the split, is invalid. */
#if defined(__HIPCC__)
#define LC3D_HD __host__ __device__
#else
#define LC3D_HD
#endif
enum { LC3D_FRAME_GOOD = 0, LC3D_FRAME_LOST = 1, LC3D_FRAME_BAD_FLAG = 2, LC3D_FRAME_BAD_SIZE = 3 };
#define LC3D_DEC_ST_INVALID 2            /* status bit of lc3plus_dec_batch_decode_sizes_device: concealed because the size or flag was invalid */
static inline LC3D_HD int lc3d_dec_frame_class(int nb, int bfi, int in_stride, const lc3d_dchan* tab, int tab_n, int channels)
{
    if (bfi > 1) return LC3D_FRAME_BAD_FLAG;
    if (bfi == 1 || nb == 0) return LC3D_FRAME_LOST;
    if (nb < 0 || nb > in_stride) return LC3D_FRAME_BAD_SIZE;
    for (int c = 0; c < channels; c++) {
        const int k = nb / channels + (c < nb % channels);
        if (k >= tab_n || k == 0 || tab[k].nbytes != k) return LC3D_FRAME_BAD_SIZE;
    }
    return LC3D_FRAME_GOOD;
}

/* The same rule for frames packed back to back (lc3plus_dec_batch_decode_packed): in place of in_stride, a good frame also lies inside the buffer
 * (0 <= off, off + nb <= cap) and is at most max_bytes long.  A lost frame's size and offset are not looked at. */
static inline LC3D_HD int lc3d_dec_frame_class_packed(int nb, int bfi, long long off, long long cap, int max_bytes, const lc3d_dchan* tab, int tab_n,
                                                      int channels)
{
    if (bfi > 1) return LC3D_FRAME_BAD_FLAG;
    if (bfi == 1 || nb == 0) return LC3D_FRAME_LOST;
    if (nb < 0 || nb > max_bytes || off < 0 || off > cap - nb) return LC3D_FRAME_BAD_SIZE;
    return lc3d_dec_frame_class(nb, 0, max_bytes, tab, tab_n, channels);
}
/* Per-stream frame counts (lc3plus_dec_batch_set_frame_counts): of a call's n_frames, stream s holds the first min(max(counts[s], 0), n_frames); the frames behind
 * them are absent - not looked at, not read, neither decoded nor concealed, no PCM written, status exactly LC3D_DEC_ST_ABSENT.  On the host in
 * lc3plus_dec_plan_counts, on the device in the ragged plan kernels (lc3_dec_kernels.inc). */
#define LC3D_DEC_ST_ABSENT 8
static inline LC3D_HD int lc3d_dec_count_clamp(int count, int n_frames) { return count < 0 ? 0 : count > n_frames ? n_frames : count; }
/* The encoder's counterpart (lc3plus_enc_batch_set_frame_counts), with the same clamp: an absent frame's rate, bandwidth and placement entries are not looked at,
 * no sample of its PCM is read, it is not encoded, no byte of out is written, its num_bytes is 0 and its flags are exactly LC3D_ENC_FL_ABSENT.  On the host in
 * lc3plus_enc_plan_rates_ragged, on the device in lc3_enc_plan_rates_kernel_rag (lc3_enc_ragged.inc). */
#define LC3D_ENC_FL_ABSENT 32
/* Packed encoder output (lc3plus_enc_batch_encode_packed): a frame of nb bytes at offset off is written where it fits the caller's capacity; one that does
 * not is still encoded, but its bytes are not written and it gets LC3D_ENC_FL_PACK_CAP.  The host hook lc3plus_plan_packed and lc3_pack_offsets_kernel. */
#define LC3D_ENC_FL_PACK_CAP 8
#define LC3D_PACK_STREAM_MAJOR 0
#define LC3D_PACK_FRAME_MAJOR 1
static inline LC3D_HD int lc3d_pack_fits(long long off, int nb, long long cap) { return off >= 0 && nb >= 0 && off <= cap - nb; }

/* The bandwidth controller's words for a bandwidth of bw Hz (R/lc3.c:199-201, lc3_enc_set_bandwidth): the cut-off line and the cap on the
 * detected bandwidth index.  The host's set_bandwidth and the per-frame-bandwidth kernels (lc3plus_enc_batch_encode_bandwidths) use these. */
static inline LC3D_HD int lc3d_bw_cut_bin(int bw, int dms) { return (bw * dms) / 5000; }
static inline LC3D_HD int lc3d_bw_index(int bw) { const int i = (bw / 4000) - 1; return i > 0 ? i : 0; }

/* The per-frame rules of the encoder's per-frame rates and bandwidths, one stream-frame at a time, on the host (lc3_host.c: enc_plan_bitrates,
 * enc_plan_bandwidths, the test hook lc3plus_enc_plan_rates_lenient) and on the device (lc3_enc_plan_rates_kernel). */
#define LC3D_ENC_FL_RATE 1               /* flag bits of lc3plus_enc_batch_encode_rates_device: the rate was refused, the frame keeps the carried rate */
#define LC3D_ENC_FL_BW_REFUSED 2         /* the bandwidth was refused as set_bandwidth refuses it (2 * bw > min(fs_in, 40000)): the value in force stays */
#define LC3D_ENC_FL_BW_RANGE 4           /* the bandwidth is negative or its cut-off line is below 1: the value in force stays */
/* Rate br of a stream-frame -> its bytes (all channels), as derive_bitrate computes them (R/setup_enc_lc3.c:196-240), or -1 where set_bitrate refuses
 * the rate (outside [lo, hi], the geometry's limits), a channel's share falls outside the table 1 ... max_chan, or the bytes exceed lim.  br is
 * compared with the limits before it is multiplied: hi * N < 2^31 for every geometry. */
static inline LC3D_HD int lc3d_enc_rate_bytes(int br, int lo, int hi, int N, int fs_in, int channels, int max_chan, int lim)
{
    if (br <= 0 || br < lo || br > hi) return -1;
    const int tb = br * N / (8 * fs_in);
    if (tb / channels < 1 || (tb + channels - 1) / channels > max_chan || tb > lim) return -1;
    return tb;
}
/* Bandwidth v for a stream-frame whose bandwidth in force is *cur (lc3_enc_set_bandwidth, R/lc3.c:187-208, with half = min(fs_in, 40000) / 2 and the
 * frame length in dms): a value equal to *cur changes nothing; a negative one, or one whose cut-off line is below 1, is out of range
 * (LC3D_ENC_FL_BW_RANGE, lc3d_bw_value_ok); one above half is refused (LC3D_ENC_FL_BW_REFUSED); any other becomes *cur.  Returns the flag bits, 0 for a clean frame. */
static inline LC3D_HD int lc3d_bw_value_ok(int bw, int dms) { return bw == 0 || (bw > 0 && bw >= (5000 + dms - 1) / dms); }  /* cut-off line >= 1, no overflow */
static inline LC3D_HD int lc3d_enc_bw_step(int* cur, int v, int half, int dms)
{
    if (v == *cur) return 0;
    if (!lc3d_bw_value_ok(v, dms)) return LC3D_ENC_FL_BW_RANGE;
    if (v > half) return LC3D_ENC_FL_BW_REFUSED;
    *cur = v;
    return 0;
}
/* the geometry's constants of both rules (a kernel argument) */
typedef struct { int32_t lo, hi, N, fs_in, channels, max_chan, lim, half, dms; } lc3d_rate_rule;
/* One stream-frame of lc3plus_enc_batch_encode_rates_device: the rate br (when has_rate) and then the bandwidth bw (when has_bw), as encode_bandwidths
 * applies set_bitrate and then set_bandwidth.  The carry (*rate, *bytes: the stream's rate and its bytes; *cur_bw: the bandwidth in force) moves with
 * every value the rules accept; a refused value leaves it.  Returns the frame's LC3D_ENC_FL_* bits. */
static inline LC3D_HD int lc3d_enc_frame_step(const lc3d_rate_rule* r, int has_rate, int br, int has_bw, int bw, int* rate, int* bytes, int* cur_bw)
{
    int f = 0;
    if (has_rate) {
        const int tb = lc3d_enc_rate_bytes(br, r->lo, r->hi, r->N, r->fs_in, r->channels, r->max_chan, r->lim);
        if (tb < 0) f = LC3D_ENC_FL_RATE;
        else { *rate = br; *bytes = tb; }
    }
    if (has_bw) f |= lc3d_enc_bw_step(cur_bw, bw, r->half, r->dms);
    return f;
}

/* decoder state words per channel-stream */
#define DST_IMEM   0                                   /* 600: IMDCT overlap memory (300 used by the standard layout) */
#define DST_QPREV  600                                 /* 960: last good spectrum (concealment) */
#define DST_LY     1560                                /* 864: LTPF output history */
#define DST_LX     (1560 + DEC_LY)                     /* 16 : LTPF input history */
#define DST_SCAL   (1560 + DEC_LY + DEC_LX)            /* 16 scalars */
#define DST_WORDS  (1560 + DEC_LY + DEC_LX + 16)
/* hand-over between the two encoder kernels (lc3_encode_kernel -> lc3_enc_pack_kernel, lc3_enc_pack.inc), per channel-frame in HBM */
#define PK_RES 64                        /* [0..55] the encoder's isc[] scalars; [64..223] residual bits, LSB first (the LSB-mode list in LSB mode) */
#define PK_XQ  224                       /* quantised spectrum up to lastnz: one word per 2-tuple (int16 pairs), or int32 lines in high-resolution mode */
#define PK_STRIDE(N, hr) (PK_XQ + ((hr) ? ((N) > 480 ? 960 : 480) : ((N) > 480 ? 480 : 240)))
/* hand-over between the two decoder kernels (lc3_dec_parse.inc -> lc3_dec_kernels.inc), both in HBM */
#define PR_WORDS 112                     /* per channel-frame record: isc[0..38] of the decoder (side information), [39] = bfi after parsing, [44..45] LTPF configuration, [48..111] = the 64 SNS band gains */
#define PR_GAINS 48
#define PR_PLC 40                        /* lost frames: [40] nbLostCmpt, [41] cumulative attenuation (float), [42] first seed, [43] last good frame of the launch or -1 */
#define OV_ROW_STD 480                    /* transformed frame in HBM: the N samples of the time-domain aliasing buffer (R/imdct.c:34-44), standard layout */
#define OV_ROW_BIG 960                    /* large layout */
#define PR_BFI 39
#define PR_LTPF 44                       /* the frame's LTPF configuration, written by the concealment kernel: [44] ltpf_beta (float), [45] ltpf_beta_idx (frame sizes can change per frame) */
#define WS_ROW(N) ((N) > 480 ? 960 : 480)  /* per channel-frame spectrum row (words) */
enum { DS_PITCH_INT = 0, DS_PITCH_FR, DS_BETA_IDX, DS_PARAM0, DS_PARAM1, DS_PARAM2, DS_GAIN /* float */, DS_NBLOST, DS_CUM_ALPHA /* float */, DS_PLC_SEED,
       DS_PREV_BFI, DS_PREVPREV_BFI };

/* ---- The PCM format word of the batch calls (include/lc3plus_batch.h: LC3PLUS_PCM_*) --------------------------------------------------------------
 * Bits 0 ... 7: the sample type - 16, 24, 32 (integers as the reference's bitdepth / bps), LC3D_PCM_FLOAT32 (IEEE float, full scale 1.0) or one of the five
 * wire types LC3D_PCM_S16_BE ... LC3D_PCM_ALAW (below); bits 8, 9: the layout - none = [stream][frame][channel][sample], LC3D_PCM_INTERLEAVED =
 * [stream][time][channel], LC3D_PCM_CHANNEL_MAJOR = [stream][channel][time], time = frame * N + sample.  The same arithmetic on the host
 * (lc3plus_pcm_format_check, lc3plus_pcm_offset) and in every kernel that touches PCM: lc3d_pcm_frame gives the element index of sample 0 of (stream, frame,
 * channel); sample i is lc3d_pcm_stride further per step, and the same channel's next frame lc3d_pcm_fstep further.  An element is lc3d_pcm_elem_bytes bytes. */
#define LC3D_PCM_FLOAT32       0x80
#define LC3D_PCM_S16_BE        0x81      /* 2 bytes, big-endian: stands for 16 */
#define LC3D_PCM_S24_3LE       0x82      /* 3 bytes, little-endian two's complement: stands for 24 */
#define LC3D_PCM_S24_3BE       0x83      /* 3 bytes, big-endian: stands for 24 */
#define LC3D_PCM_ULAW          0x84      /* 1 byte, G.711 mu-law: stands for 16 */
#define LC3D_PCM_ALAW          0x85      /* 1 byte, G.711 A-law: stands for 16 */
#define LC3D_PCM_TYPE_MASK     0xff
#define LC3D_PCM_INTERLEAVED   0x100
#define LC3D_PCM_CHANNEL_MAJOR 0x200
#define LC3D_PCM_LAYOUT_MASK   0x300
static inline LC3D_HD int lc3d_pcm_type_wire(int ty) { return ty >= LC3D_PCM_S16_BE && ty <= LC3D_PCM_ALAW; }
static inline LC3D_HD int lc3d_pcm_format_ok(int fmt)
{
    const int ty = fmt & LC3D_PCM_TYPE_MASK, lay = fmt & LC3D_PCM_LAYOUT_MASK;
    if (fmt & ~(LC3D_PCM_TYPE_MASK | LC3D_PCM_LAYOUT_MASK)) return 0;
    if (ty != 16 && ty != 24 && ty != 32 && ty != LC3D_PCM_FLOAT32 && !lc3d_pcm_type_wire(ty)) return 0;
    return lay != LC3D_PCM_LAYOUT_MASK;
}
static inline LC3D_HD int lc3d_pcm_elem_bytes(int fmt)
{
    const int ty = fmt & LC3D_PCM_TYPE_MASK;
    return ty == LC3D_PCM_ULAW || ty == LC3D_PCM_ALAW ? 1 : ty == 16 || ty == LC3D_PCM_S16_BE ? 2 : ty == LC3D_PCM_S24_3LE || ty == LC3D_PCM_S24_3BE ? 3 : 4;
}
/* The wire types' conversion rule, one text for the host functions (lc3plus_pcm_to_native / _from_native) and the kernels.  Into the encoder a wire sample
 * becomes the integer its type stands for (then R/enc_lc3_fl.c:30-42 for that depth); out of the decoder the integer output of that depth (R/dec_lc3_fl.c:115-127)
 * becomes the wire sample: bytes swapped, the 24-bit value saturated as R/tinywaveout_c.h:403-424 clips it, or compressed by G.711.
 * G.711: code c -> sample (ITU-T G.711 tables 1a / 2a at 16 bits), and sample x -> code with the magnitude taken by one's complement (y = x < 0 ? ~x : x), so that
 * -1 has magnitude 0 and both signs quantise alike. */
static inline LC3D_HD int lc3d_g711_expand(int c, int alaw)
{
    const int k = alaw ? (c ^ 0x55) : (~c & 0xff), e = (k >> 4) & 7, q = k & 15;
    if (alaw) { const int m = e == 0 ? (2 * q + 1) << 3 : ((2 * q + 33) << (e - 1)) << 3; return (k & 0x80) ? m : -m; }
    const int m = ((2 * q + 33) << (e + 2)) - 132;
    return (c & 0x80) ? m : -m;
}
static inline LC3D_HD int lc3d_g711_compress(int x /* int16 */, int alaw)
{
    const int s = x < 0, y = s ? ~x : x;
    if (alaw) {
        const int m = y >> 4;
        int c7 = m;
        if (m > 15) { const int e = 28 - __builtin_clz((unsigned)m); c7 = (e << 4) | ((m >> (e - 1)) & 15); }
        return (c7 | (s ? 0 : 0x80)) ^ 0x55;
    }
    int a = (y >> 2) + 33;
    if (a > 8191) a = 8191;
    const int e = 26 - __builtin_clz((unsigned)a), q = (a >> (e + 1)) & 15;
    return (s ? 0 : 0x80) | ((7 - e) << 4) | (15 - q);
}
static inline LC3D_HD int32_t lc3d_pcm_sat24(int32_t v) { return v > 8388607 ? 8388607 : v < -8388608 ? -8388608 : v; }
static inline LC3D_HD int lc3d_pcm_stride(int fmt, int channels) { return (fmt & LC3D_PCM_INTERLEAVED) ? channels : 1; }
static inline LC3D_HD size_t lc3d_pcm_fstep(int fmt, int channels, int N) { return (fmt & LC3D_PCM_CHANNEL_MAJOR) ? (size_t)N : (size_t)N * channels; }
static inline LC3D_HD size_t lc3d_pcm_frame(int fmt, int channels, int T, int N, int strm, int t, int ch)
{
    if (fmt & LC3D_PCM_CHANNEL_MAJOR) return (((size_t)strm * channels + ch) * T + t) * N;
    if (fmt & LC3D_PCM_INTERLEAVED) return ((size_t)strm * T + t) * N * channels + ch;
    return (((size_t)strm * T + t) * channels + ch) * N;
}

/* ---- Placed PCM (lc3plus_{enc,dec}_batch_set_pcm_placement) --------------------------------------------------------------------------------------
 * In place of lc3d_pcm_frame: frame (stream, t) of a call lies at the element offset off = offsets[stream * T + t], read from device memory when the call's
 * kernels run.  off is sample 0 of channel 0; the frame's channels * N elements follow each other - channel after channel with no layout bit, sample by sample
 * with LC3D_PCM_INTERLEAVED (there is no channel-major placement: that layout's channel distance belongs to a dense call).  A frame is valid where it lies
 * inside [0, cap); nothing of an invalid frame is touched: the encoder reads zeros for it, the decoder does not write it.  The same text on the host
 * (lc3plus_pcm_placed_offset, lc3plus_plan_placed) and in the _plc kernels. */
#define LC3D_ENC_FL_PCM_PLACE 16         /* flag bit of the encoder's device flags: the frame's PCM offset is invalid, the frame was encoded as silence */
#define LC3D_DEC_ST_PCM_PLACE 4          /* status bit of the decoder's device status: the frame's PCM offset is invalid, its PCM was not written */
static inline LC3D_HD int lc3d_pcm_placed_ok(long long off, int channels, int N, long long cap)
{
    const long long fe = (long long)channels * N;
    return off >= 0 && cap >= fe && off <= cap - fe;         /* no overflow: cap - fe >= 0 */
}
static inline LC3D_HD size_t lc3d_pcm_placed_frame(int fmt, int channels, int N, long long off, int ch)
{
    (void)channels;
    return (size_t)off + ((fmt & LC3D_PCM_INTERLEAVED) ? (size_t)ch : (size_t)ch * (size_t)N);
}

#endif
