/* lc3_kernel_decls.h -- every kernel the host runtime (lc3_runtime.hip) launches, declared once.  lc3_kernels.hip includes this file too, in every one of its
 * objects: a kernel is extern "C", so a definition whose parameters differ from its declaration here does not compile - without that a mismatch would
 * be a kernel reading the wrong pointer.  Kernels with the same parameters share one LC3_*_ARGS list.  Needs <hip/hip_runtime.h> and lc3_launch.h. */
#ifndef LC3_KERNEL_DECLS_H
#define LC3_KERNEL_DECLS_H
#include "lc3_shim.h"
#include "lc3_launch.h"

/* ---- the one-wave encode kernels (lc3_enc_wave.inc), one per object of lc3_kernels.hip ----
 * The parameters every one of them takes ... */
#define LC3_OW_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, float* __restrict__ state, const void* __restrict__ pcm, int bitdepth, int T, \
    uint8_t* __restrict__ out, int out_stride, int ncs, lc3d_trace* __restrict__ trace, \
    int* __restrict__ dump /* [cs][T][dstride] hand-over to lc3_enc_pack_kernel, or null: write the bytes here */, int dstride, \
    const float* __restrict__ y12 /* [cs][T][128] HP-filtered 12.8 kHz signal from the pre-kernels, or null: resample here */, \
    uint8_t* __restrict__ status /* [cs][dT] LC3D_ENC_ST_* bits (zeroed by the host), or null */, \
    int dT, int dt0 /* the hand-over and the status rows hold dT frames per channel-stream; this launch's frame t is their frame dt0 + t */, \
    const float* __restrict__ spec /* [cs][T][N] MDCT spectra from lc3_enc_front_kernel, or null: transform here */, \
    const float* __restrict__ frec /* [cs][T][FR_WORDS] with the SNS result of lc3_enc_snsvq_kernel */, \
    const float* __restrict__ xnext /* [cs][MEMCAP] MDCT memory after the last frame */
/* ... and the three optional groups behind them, in this order: per-frame bitrates (var), per-frame bandwidths (vbw), packed output (pk).  LC3_OW_ARGS_* are the
 * parameters of a group; the runtime defines LC3_OW_VALS_* with the values it passes; LC3_OW_OPT puts the groups a kernel takes (1) in order for either. */
#define LC3_OW_ARGS_VAR_0
#define LC3_OW_ARGS_VAR_1 , const uint16_t* __restrict__ fsz /* [stream][dT] bytes of each stream-frame */, const lc3d_chan* __restrict__ etab /* per channel byte count */
#define LC3_OW_ARGS_VBW_0
#define LC3_OW_ARGS_VBW_1 , const uint16_t* __restrict__ bwf /* [stream][dT] bandwidth in force for each stream-frame, Hz */
#define LC3_OW_ARGS_PK_0
#define LC3_OW_ARGS_PK_1 , const long long* __restrict__ poff /* [stream][dT] byte offset of each stream-frame in out, -1: not written */
/* the two parameters every placed kernel (_plc: lc3_plan.h lc3d_pcm_placed_*, lc3_kernels.hip pcm_placed_load) takes behind those of its dense twin */
#define LC3_PLACED_ARGS , const long long* __restrict__ plo /* [stream][T] element offset of each stream-frame's PCM */, long long plcap /* length of the PCM buffer, elements */
/* the parameter every ragged kernel (_rag: lc3_dec_kernels.inc DEC_TC, lc3_enc_wave.inc ENC_TC) takes behind those of its dense twin, behind the placed ones where it has both */
#define LC3_RAGGED_ARGS , const int32_t* __restrict__ cnt /* [stream] frames of each stream present in this call, clamped to 0 ... T */
#define LC3_OW_OPT_(G, var, vbw, pk) G##VAR_##var G##VBW_##vbw G##PK_##pk
#define LC3_OW_OPT(G, var, vbw, pk) LC3_OW_OPT_(G, var, vbw, pk)
/* The variants: X(name, large layout, var, vbw, pk), each once more named name_fmt for the PCM formats beyond 16 / 24 / 32, name_wire for the wire sample types and name_plc for placed PCM.  There is no large-layout kernel
 * with per-frame bandwidths: that layout only serves 96 kHz, which is high-resolution and has no bandwidth controller. */
#define LC3_OW_KERNELS(X) \
    X(lc3_encode_kernel,            0, 0, 0, 0) X(lc3_encode_kernel_pk,            0, 0, 0, 1) \
    X(lc3_encode_kernel_big,        1, 0, 0, 0) X(lc3_encode_kernel_big_pk,        1, 0, 0, 1) \
    X(lc3_encode_kernel_var,        0, 1, 0, 0) X(lc3_encode_kernel_var_pk,        0, 1, 0, 1) \
    X(lc3_encode_kernel_big_var,    1, 1, 0, 0) X(lc3_encode_kernel_big_var_pk,    1, 1, 0, 1) \
    X(lc3_encode_kernel_vbw,        0, 0, 1, 0) X(lc3_encode_kernel_vbw_pk,        0, 0, 1, 1) \
    X(lc3_encode_kernel_var_vbw,    0, 1, 1, 0) X(lc3_encode_kernel_var_vbw_pk,    0, 1, 1, 1)
#define LC3_OW_DECL(name, big, var, vbw, pk) \
    extern "C" __global__ void name(LC3_OW_ARGS LC3_OW_OPT(LC3_OW_ARGS_, var, vbw, pk)), name##_fmt(LC3_OW_ARGS LC3_OW_OPT(LC3_OW_ARGS_, var, vbw, pk)), \
        name##_wire(LC3_OW_ARGS LC3_OW_OPT(LC3_OW_ARGS_, var, vbw, pk)), name##_plc(LC3_OW_ARGS LC3_OW_OPT(LC3_OW_ARGS_, var, vbw, pk) LC3_PLACED_ARGS);
LC3_OW_KERNELS(LC3_OW_DECL)
#undef LC3_OW_DECL
/* The ragged forms (per-stream frame counts, lc3plus_enc_batch_set_frame_counts), in objects of their own.  A ragged call always has per-frame sizes and an offset
 * table - lc3_enc_plan_rates_kernel_rag writes both - so var and pk are 1 in every one: X(dense twin, large layout, var, vbw, pk), named twin_rag, twin_rag_fmt ... */
#define LC3_OW_RAG_KERNELS(X) X(lc3_encode_kernel_var_pk, 0, 1, 0, 1) X(lc3_encode_kernel_big_var_pk, 1, 1, 0, 1) X(lc3_encode_kernel_var_vbw_pk, 0, 1, 1, 1)
#define LC3_OW_RAG_DECL(name, big, var, vbw, pk) \
    extern "C" __global__ void name##_rag(LC3_OW_ARGS LC3_OW_OPT(LC3_OW_ARGS_, var, vbw, pk) LC3_RAGGED_ARGS), name##_rag_fmt(LC3_OW_ARGS LC3_OW_OPT(LC3_OW_ARGS_, var, vbw, pk) LC3_RAGGED_ARGS), \
        name##_rag_wire(LC3_OW_ARGS LC3_OW_OPT(LC3_OW_ARGS_, var, vbw, pk) LC3_RAGGED_ARGS), name##_rag_plc(LC3_OW_ARGS LC3_OW_OPT(LC3_OW_ARGS_, var, vbw, pk) LC3_PLACED_ARGS LC3_RAGGED_ARGS);
LC3_OW_RAG_KERNELS(LC3_OW_RAG_DECL)
#undef LC3_OW_RAG_DECL

extern "C" {
/* ---- the encoder's pipeline (lc3_enc_*.inc), in alphabetical order ---- */
__global__ void lc3_enc_attack_kernel(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, float* __restrict__ state, int state_words, int scal_off,
    float* __restrict__ rec, int RT, int r0, int tb, int nt, int ncs);
#define LC3_FRONT4_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, const float* __restrict__ state, const void* __restrict__ pcm, int bitdepth, \
    int T, int tb, int nt, int ncs, float* __restrict__ spec, int srow, int RT, int r0, float* __restrict__ rec, float* __restrict__ xnext, \
    const float* __restrict__ xprev, int xprev_stride
__global__ void lc3_enc_front4_kernel(LC3_FRONT4_ARGS), lc3_enc_front4_kernel_fmt(LC3_FRONT4_ARGS), lc3_enc_front4_kernel_wire(LC3_FRONT4_ARGS),
    lc3_enc_front4_kernel_plc(LC3_FRONT4_ARGS LC3_PLACED_ARGS);
#define LC3_FRONT_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, const float* __restrict__ state, const void* __restrict__ pcm, int bitdepth, \
    int T, int tb, int nt, int fpw, int ncs, float* __restrict__ spec, int srow, int RT, int r0, float* __restrict__ rec, float* __restrict__ xnext, \
    const float* __restrict__ xprev, int xprev_stride, int do_scf
__global__ void lc3_enc_front_kernel(LC3_FRONT_ARGS), lc3_enc_front_kernel_big(LC3_FRONT_ARGS), lc3_enc_front_kernel_big_fmt(LC3_FRONT_ARGS),
    lc3_enc_front_kernel_fmt(LC3_FRONT_ARGS), lc3_enc_front_kernel_wire(LC3_FRONT_ARGS), lc3_enc_front_kernel_big_wire(LC3_FRONT_ARGS),
    lc3_enc_front_kernel_plc(LC3_FRONT_ARGS LC3_PLACED_ARGS), lc3_enc_front_kernel_big_plc(LC3_FRONT_ARGS LC3_PLACED_ARGS);
#define LC3_FRONTM_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, const float* __restrict__ state, const void* __restrict__ pcm, int bitdepth, \
    int T, int tb, int nt, int F, int ncs, float* __restrict__ spec, int srow, int RT, int r0, float* __restrict__ rec, float* __restrict__ xnext, \
    const float* __restrict__ xprev, int xprev_stride
__global__ void lc3_enc_frontm_kernel(LC3_FRONTM_ARGS), lc3_enc_frontm_kernel_fmt(LC3_FRONTM_ARGS), lc3_enc_frontm_kernel_wire(LC3_FRONTM_ARGS),
    lc3_enc_frontm_kernel_plc(LC3_FRONTM_ARGS LC3_PLACED_ARGS);
__global__ void lc3_enc_hp50_kernel(const lc3d_plan* __restrict__ P, float* __restrict__ state, int state_words, int scal_off, int T, int tb, int nt, int ncs,
    float* __restrict__ d12);
#define LC3_PACK_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int* __restrict__ dump, int dstride, int T, int tb, int nt, int ncs, \
    uint8_t* __restrict__ out, int out_stride, uint8_t* __restrict__ status, float* __restrict__ rows, int srow, const float* __restrict__ frec, int skip_bytes
__global__ void lc3_enc_pack_code_kernel(LC3_PACK_ARGS), lc3_enc_pack_head_kernel(LC3_PACK_ARGS), lc3_enc_pack_kernel(LC3_PACK_ARGS),
    lc3_enc_pack_kernel_w5(LC3_PACK_ARGS);
#define LC3_PACK_PK_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int* __restrict__ dump, int dstride, int T, int tb, int nt, int ncs, \
    uint8_t* __restrict__ out, int out_stride, uint8_t* __restrict__ status, float* __restrict__ rows, int srow, const float* __restrict__ frec, int skip_bytes, \
    const long long* __restrict__ poff
__global__ void lc3_enc_pack_code_kernel_pk(LC3_PACK_PK_ARGS), lc3_enc_pack_head_kernel_pk(LC3_PACK_PK_ARGS), lc3_enc_pack_kernel_pk(LC3_PACK_PK_ARGS),
    lc3_enc_pack_kernel_w5_pk(LC3_PACK_PK_ARGS);
#define LC3_PITCH_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, float* __restrict__ state, int state_words, int memcap, \
    const float* __restrict__ y12, int T, int t0, int nt, int ncs, float* __restrict__ frec, int RT, int r0
__global__ void lc3_enc_pitch2_kernel(LC3_PITCH_ARGS), lc3_enc_pitch2_kernel_l32(LC3_PITCH_ARGS), lc3_enc_pitch2_kernel_l64(LC3_PITCH_ARGS),
    lc3_enc_pitch_kernel(LC3_PITCH_ARGS);
#define LC3_RATE_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, float* __restrict__ state, int T, int t0, int nt, int ncs, \
    const float* __restrict__ rows, int srow, float* __restrict__ frec, const float* __restrict__ xnext, int last
__global__ void lc3_enc_rate_kernel(LC3_RATE_ARGS), lc3_enc_rate_kernel_big(LC3_RATE_ARGS);
__global__ void lc3_enc_resample48_kernel(const lc3d_plan* __restrict__ P, const int16_t* __restrict__ pcm, int channels, int memcap, int T, int tb, int nt, int ncs,
    float* __restrict__ d12, const float* __restrict__ xprev, int xprev_stride);
__global__ void lc3_enc_resample48f_kernel(const lc3d_plan* __restrict__ P, const float* __restrict__ pcm, int fmt, int channels, int memcap, int T, int tb, int nt,
    int ncs, float* __restrict__ d12, const float* __restrict__ xprev, int xprev_stride);
__global__ void lc3_enc_resample48w_kernel(const lc3d_plan* __restrict__ P, const unsigned* __restrict__ pcm, int fmt, int channels, int memcap, int T, int tb, int nt,
    int ncs, float* __restrict__ d12, const float* __restrict__ xprev, int xprev_stride);
#define LC3_RESAMPLE96_ARGS const lc3d_plan* __restrict__ P, const int16_t* __restrict__ pcm, int channels, int memcap, int T, int tb, int nt, int ncs, \
    float* __restrict__ d12, const float* __restrict__ xprev, int xprev_stride
__global__ void lc3_enc_resample96_kernel_n240(LC3_RESAMPLE96_ARGS), lc3_enc_resample96_kernel_n480(LC3_RESAMPLE96_ARGS),
    lc3_enc_resample96_kernel_n960(LC3_RESAMPLE96_ARGS);
#define LC3_RESAMPLE_ARGS const lc3d_plan* __restrict__ P, const float* __restrict__ state, int state_words, int memcap, const void* __restrict__ pcm, int bitdepth, \
    int T, int tb, int nt, int ncs, float* __restrict__ d12, const float* __restrict__ xprev, int xprev_stride
__global__ void lc3_enc_resample_fmt_kernel(LC3_RESAMPLE_ARGS), lc3_enc_resample_kernel(LC3_RESAMPLE_ARGS), lc3_enc_resample_wire_kernel(LC3_RESAMPLE_ARGS),
    lc3_enc_resample_plc_kernel(LC3_RESAMPLE_ARGS LC3_PLACED_ARGS);
__global__ void lc3_enc_scf_lane_kernel(const lc3d_plan* __restrict__ P, int RT, int r0, int nt, int ncs, const float* __restrict__ rows, int srow,
    float* __restrict__ frec, int with_vq);
#define LC3_SHAPE_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int T, int tb, int nt, int fpw, int ncs, float* __restrict__ rows, int srow, \
    float* __restrict__ frec
__global__ void lc3_enc_shape_kernel(LC3_SHAPE_ARGS), lc3_enc_shape_kernel_big(LC3_SHAPE_ARGS);
__global__ void lc3_enc_shape_kernel_vbw(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int T, int tb, int nt, int fpw, int ncs,
    float* __restrict__ rows, int srow, float* __restrict__ frec, const uint16_t* __restrict__ bwf);
__global__ void lc3_enc_shape_lane_kernel(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int RT, int r0, int nt, int ncs, float* __restrict__ rows,
    int srow, float* __restrict__ frec);
__global__ void lc3_enc_shape_lane_kernel_vbw(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int RT, int r0, int nt, int ncs,
    float* __restrict__ rows, int srow, float* __restrict__ frec, const uint16_t* __restrict__ bwf);
__global__ void lc3_enc_snsvq_kernel(const lc3d_plan* __restrict__ P, float* __restrict__ rec, int RT, int r0, int tb, int nt, int ncs, int with_attack);
#define LC3_TAILW_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int T, int nt, int fpw, int ncs, const float* __restrict__ rows, int srow, \
    const float* __restrict__ frec, uint8_t* __restrict__ out, int out_stride, uint8_t* __restrict__ status, int min_bytes
__global__ void lc3_enc_tailw_kernel(LC3_TAILW_ARGS), lc3_enc_tailw_kernel_big(LC3_TAILW_ARGS);
/* the ragged forms of the pipelined path (per-stream frame counts, lc3plus_enc_batch_set_frame_counts; standard layout), in objects of their own: every step's twin
 * with LC3_RAGGED_ARGS behind the twin's parameters.  The writers are the _pk forms (a ragged call always has a table of offsets); the typed resamplers, pitch2, the
 * wave-per-frame shape kernel, the split and frame-per-wave writers and the large layout have none. */
__global__ void lc3_enc_attack_kernel_rag(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, float* __restrict__ state, int state_words, int scal_off,
    float* __restrict__ rec, int RT, int r0, int tb, int nt, int ncs LC3_RAGGED_ARGS);
__global__ void lc3_enc_front4_kernel_rag(LC3_FRONT4_ARGS LC3_RAGGED_ARGS), lc3_enc_front4_kernel_fmt_rag(LC3_FRONT4_ARGS LC3_RAGGED_ARGS),
    lc3_enc_front4_kernel_wire_rag(LC3_FRONT4_ARGS LC3_RAGGED_ARGS), lc3_enc_front4_kernel_plc_rag(LC3_FRONT4_ARGS LC3_PLACED_ARGS LC3_RAGGED_ARGS);
__global__ void lc3_enc_front_kernel_rag(LC3_FRONT_ARGS LC3_RAGGED_ARGS), lc3_enc_front_kernel_fmt_rag(LC3_FRONT_ARGS LC3_RAGGED_ARGS),
    lc3_enc_front_kernel_wire_rag(LC3_FRONT_ARGS LC3_RAGGED_ARGS), lc3_enc_front_kernel_plc_rag(LC3_FRONT_ARGS LC3_PLACED_ARGS LC3_RAGGED_ARGS);
__global__ void lc3_enc_frontm_kernel_rag(LC3_FRONTM_ARGS LC3_RAGGED_ARGS), lc3_enc_frontm_kernel_fmt_rag(LC3_FRONTM_ARGS LC3_RAGGED_ARGS),
    lc3_enc_frontm_kernel_wire_rag(LC3_FRONTM_ARGS LC3_RAGGED_ARGS), lc3_enc_frontm_kernel_plc_rag(LC3_FRONTM_ARGS LC3_PLACED_ARGS LC3_RAGGED_ARGS);
__global__ void lc3_enc_hp50_kernel_rag(const lc3d_plan* __restrict__ P, float* __restrict__ state, int state_words, int scal_off, int T, int tb, int nt, int ncs,
    float* __restrict__ d12 LC3_RAGGED_ARGS);
__global__ void lc3_enc_pack_kernel_pk_rag(LC3_PACK_PK_ARGS LC3_RAGGED_ARGS), lc3_enc_pack_kernel_w5_pk_rag(LC3_PACK_PK_ARGS LC3_RAGGED_ARGS);
__global__ void lc3_enc_pitch_kernel_rag(LC3_PITCH_ARGS LC3_RAGGED_ARGS);
__global__ void lc3_enc_rate_kernel_rag(LC3_RATE_ARGS LC3_RAGGED_ARGS);
__global__ void lc3_enc_resample_fmt_kernel_rag(LC3_RESAMPLE_ARGS LC3_RAGGED_ARGS), lc3_enc_resample_kernel_rag(LC3_RESAMPLE_ARGS LC3_RAGGED_ARGS),
    lc3_enc_resample_wire_kernel_rag(LC3_RESAMPLE_ARGS LC3_RAGGED_ARGS), lc3_enc_resample_plc_kernel_rag(LC3_RESAMPLE_ARGS LC3_PLACED_ARGS LC3_RAGGED_ARGS);
__global__ void lc3_enc_scf_lane_kernel_rag(const lc3d_plan* __restrict__ P, int RT, int r0, int nt, int ncs, const float* __restrict__ rows, int srow,
    float* __restrict__ frec, int with_vq LC3_RAGGED_ARGS);
__global__ void lc3_enc_shape_lane_kernel_rag(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int RT, int r0, int nt, int ncs, float* __restrict__ rows,
    int srow, float* __restrict__ frec LC3_RAGGED_ARGS);
__global__ void lc3_enc_shape_lane_kernel_vbw_rag(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int RT, int r0, int nt, int ncs,
    float* __restrict__ rows, int srow, float* __restrict__ frec, const uint16_t* __restrict__ bwf LC3_RAGGED_ARGS);
__global__ void lc3_enc_snsvq_kernel_rag(const lc3d_plan* __restrict__ P, float* __restrict__ rec, int RT, int r0, int tb, int nt, int ncs, int with_attack LC3_RAGGED_ARGS);
/* ---- the decoder (lc3_dec_*.inc) ---- */
__global__ void lc3_dec_imdct4_kernel(const lc3d_plan* __restrict__ P, const float* __restrict__ state, const int* __restrict__ rec, const float* __restrict__ ws, int T,
    int ncs, float* __restrict__ ov);
#define LC3_DEC_IMDCT_ARGS const lc3d_plan* __restrict__ P, const float* __restrict__ state, const int* __restrict__ rec, const float* __restrict__ ws, int T, int ncs, \
    float* __restrict__ ov, lc3d_dec_trace* __restrict__ trace
__global__ void lc3_dec_imdct_kernel(LC3_DEC_IMDCT_ARGS), lc3_dec_imdct_kernel_big(LC3_DEC_IMDCT_ARGS);
#define LC3_DEC_PARSE_ARGS const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ chans, const uint8_t* __restrict__ in, int in_stride, \
    const uint8_t* __restrict__ bfi_flags, const uint16_t* __restrict__ sizes, const lc3d_dchan* __restrict__ dtab, int T, int n_streams, int nw_max, \
    int* __restrict__ rec, float* __restrict__ ws, int wsr
__global__ void lc3_dec_parse_kernel(LC3_DEC_PARSE_ARGS), lc3_dec_parse_kernel_g(LC3_DEC_PARSE_ARGS), lc3_dec_parse_kernel_g_var(LC3_DEC_PARSE_ARGS),
    lc3_dec_parse_kernel_var(LC3_DEC_PARSE_ARGS);
#define LC3_DEC_PARSE_PK_ARGS const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ chans, const uint8_t* __restrict__ in, const long long* __restrict__ offs, \
    const uint8_t* __restrict__ bfi_flags, const uint16_t* __restrict__ sizes, const lc3d_dchan* __restrict__ dtab, int T, int n_streams, int nw_max, \
    int* __restrict__ rec, float* __restrict__ ws, int wsr
__global__ void lc3_dec_parse_kernel_g_var_pk(LC3_DEC_PARSE_PK_ARGS), lc3_dec_parse_kernel_var_pk(LC3_DEC_PARSE_PK_ARGS);
__global__ void lc3_dec_plan_packed_kernel(const int32_t* __restrict__ num_bytes, const long long* __restrict__ offs, const uint8_t* __restrict__ bfi,
    const lc3d_dchan* __restrict__ dtab, int tab_n, int channels, long long cap, int max_bytes, long long n, uint16_t* __restrict__ sizes, uint8_t* __restrict__ lost,
    uint8_t* __restrict__ invalid);
__global__ void lc3_dec_plan_sizes_kernel(const int32_t* __restrict__ num_bytes, const uint8_t* __restrict__ bfi, const lc3d_dchan* __restrict__ dtab, int tab_n,
    int channels, int in_stride, long long n, uint16_t* __restrict__ sizes, uint8_t* __restrict__ lost, uint8_t* __restrict__ invalid);
__global__ void lc3_dec_plc_kernel(const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ chans, const uint16_t* __restrict__ sizes,
    const lc3d_dchan* __restrict__ dtab, float* __restrict__ state, int* __restrict__ rec, int T, int ncs);
__global__ void lc3_dec_sizes_tail_kernel(const uint16_t* __restrict__ sizes, const uint8_t* __restrict__ invalid, const lc3d_dchan* __restrict__ dtab, int channels,
    int n_streams, int T, lc3d_dchan* __restrict__ chans, uint8_t* __restrict__ status);
#define LC3_DEC_SYNTH_ARGS const lc3d_plan* __restrict__ P, float* __restrict__ state, const int* __restrict__ rec, const float* __restrict__ ws, \
    const float* __restrict__ ov, int T, void* __restrict__ pcm, int bps, int ncs, uint8_t* __restrict__ status, lc3d_dec_trace* __restrict__ trace
__global__ void lc3_dec_synth_kernel(LC3_DEC_SYNTH_ARGS), lc3_dec_synth_kernel_big(LC3_DEC_SYNTH_ARGS), lc3_dec_synth_kernel_plc(LC3_DEC_SYNTH_ARGS LC3_PLACED_ARGS),
    lc3_dec_synth_kernel_big_plc(LC3_DEC_SYNTH_ARGS LC3_PLACED_ARGS);
/* the ragged forms (per-stream frame counts, lc3plus_dec_batch_set_frame_counts), in objects of their own; the parser has none (a frame of size 0 is read by no parser) */
__global__ void lc3_dec_imdct4_kernel_rag(const lc3d_plan* __restrict__ P, const float* __restrict__ state, const int* __restrict__ rec, const float* __restrict__ ws, int T,
    int ncs, float* __restrict__ ov LC3_RAGGED_ARGS);
__global__ void lc3_dec_imdct_kernel_rag(LC3_DEC_IMDCT_ARGS LC3_RAGGED_ARGS), lc3_dec_imdct_kernel_big_rag(LC3_DEC_IMDCT_ARGS LC3_RAGGED_ARGS);
__global__ void lc3_dec_plan_packed_kernel_rag(const int32_t* __restrict__ num_bytes, const long long* __restrict__ offs, const uint8_t* __restrict__ bfi,
    const lc3d_dchan* __restrict__ dtab, int tab_n, int channels, long long cap, int max_bytes, long long n, uint16_t* __restrict__ sizes, uint8_t* __restrict__ lost,
    uint8_t* __restrict__ invalid, const int32_t* __restrict__ counts, int T, int32_t* __restrict__ cnt);
__global__ void lc3_dec_plan_sizes_kernel_rag(const int32_t* __restrict__ num_bytes, const uint8_t* __restrict__ bfi, const lc3d_dchan* __restrict__ dtab, int tab_n,
    int channels, int in_stride, long long n, uint16_t* __restrict__ sizes, uint8_t* __restrict__ lost, uint8_t* __restrict__ invalid,
    const int32_t* __restrict__ counts, int T, int32_t* __restrict__ cnt);
__global__ void lc3_dec_plc_kernel_rag(const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ chans, const uint16_t* __restrict__ sizes,
    const lc3d_dchan* __restrict__ dtab, float* __restrict__ state, int* __restrict__ rec, int T, int ncs LC3_RAGGED_ARGS);
__global__ void lc3_dec_sizes_tail_kernel_rag(const uint16_t* __restrict__ sizes, const uint8_t* __restrict__ invalid, const lc3d_dchan* __restrict__ dtab, int channels,
    int n_streams, int T, lc3d_dchan* __restrict__ chans, uint8_t* __restrict__ status, const int32_t* __restrict__ cnt, const long long* __restrict__ plo,
    long long plcap, int N);
__global__ void lc3_dec_synth_kernel_rag(LC3_DEC_SYNTH_ARGS LC3_RAGGED_ARGS), lc3_dec_synth_kernel_big_rag(LC3_DEC_SYNTH_ARGS LC3_RAGGED_ARGS),
    lc3_dec_synth_kernel_rag_plc(LC3_DEC_SYNTH_ARGS LC3_PLACED_ARGS LC3_RAGGED_ARGS), lc3_dec_synth_kernel_big_rag_plc(LC3_DEC_SYNTH_ARGS LC3_PLACED_ARGS LC3_RAGGED_ARGS);
/* ---- stream lifecycle, per-frame plans, packed offsets, test hook (lc3_util_kernels.inc) ---- */
__global__ void lc3_enc_plan_rates_kernel(lc3d_rate_rule r, const int32_t* __restrict__ rates, const int32_t* __restrict__ bws, int T, int n_streams,
    int4* __restrict__ carry, const lc3d_chan* __restrict__ seed, uint16_t* __restrict__ fsz, uint16_t* __restrict__ bwf, int32_t* __restrict__ num_bytes,
    uint8_t* __restrict__ flags, int4* __restrict__ pend, int vec4);
__global__ void lc3_enc_rates_tail_kernel(const int4* __restrict__ pend, const lc3d_chan* __restrict__ etab, lc3d_chan* __restrict__ chans, int channels, int ncs,
    int dms, int all);
/* the encoder's ragged calls (lc3_enc_ragged.inc) */
__global__ void lc3_enc_plan_rates_kernel_rag(lc3d_rate_rule r, const int32_t* __restrict__ rates, const int32_t* __restrict__ bws, int T, int n_streams,
    int4* __restrict__ carry, const lc3d_chan* __restrict__ seed, uint16_t* __restrict__ fsz, uint16_t* __restrict__ bwf, int32_t* __restrict__ num_bytes,
    uint8_t* __restrict__ flags, int4* __restrict__ pend, int vec4, const int32_t* __restrict__ counts, int32_t* __restrict__ cnt, long long* __restrict__ tab,
    int out_stride);
__global__ void lc3_enc_rates_tail_kernel_rag(const int4* __restrict__ pend, const lc3d_chan* __restrict__ etab, lc3d_chan* __restrict__ chans, int channels, int ncs,
    int dms, int all, const int32_t* __restrict__ cnt);
__global__ void lc3_enc_absent_kernel(const int32_t* __restrict__ cnt, int T, long long n, uint8_t* __restrict__ flags);
__global__ void lc3_fastmath_test_kernel(int kind, const float* __restrict__ x, float* __restrict__ y, long long n);
__global__ void lc3_pcm_placed_mark_kernel(const long long* __restrict__ plo, long long plcap, int channels, int N, long long n, uint8_t* __restrict__ out, int bit);
__global__ void lc3_pack_base_kernel(long long* __restrict__ bsum, long long nb, long long* __restrict__ total);
__global__ void lc3_pack_offsets_kernel(PkSrc q, long long n, const long long* __restrict__ base, long long cap, long long* __restrict__ tab,
    long long* __restrict__ offsets, uint8_t* __restrict__ flags, int plan_flags, int32_t* __restrict__ num_bytes);
__global__ void lc3_pack_sums_kernel(PkSrc q, long long n, long long* __restrict__ bsum);
__global__ void lc3_stream_state_kernel(int mode, float* __restrict__ state, int row_words, int channels, const int* __restrict__ list, int n,
    const float* __restrict__ tmpl, uint8_t* __restrict__ blob, uint32_t h0, uint32_t h1, uint32_t h2, uint32_t h3, uint8_t* __restrict__ status,
    const uint32_t* __restrict__ cfg, uint32_t* __restrict__ chans, int cfg_words);
}
#endif
