/* lc3_shim.h -- the thin C-ABI between the host C code (lc3_host.c) and the HIP side (lc3_runtime.hip, which launches the kernels of lc3_kernels.hip). */
#ifndef LC3_SHIM_H
#define LC3_SHIM_H
#include <stdint.h>
#include <stddef.h>
#include "lc3_plan.h"

/* per channel-frame intermediates (debug / stage-level parity tests); same field order as oracle/lc3_oracle.h:lc3o_trace */
typedef struct {
    float spec_mdct[960]; float s12k8[129]; int T0; float normcorr; int ltpf_param[3]; int ltpf_bits; int attack;
    float ener[64]; int bw_idx; float scf[16]; int scf_idx[7]; float scf_q[16]; float spec_shaped[960];
    int tns_nfilt, tns_order[2], tns_rc_idx[16], tns_bits; float spec_tns[960];
    int target_bits_quant; float gain0; int gg_idx0, gg_min; int nbits0; float gain; int gg_idx, gain_change;
    int nbits, nbits2, lastnz, lsb_mode; int xq[960]; int fac_ns; int n_res_bits; int bp_side, mask_side;
} lc3d_trace;

/* per decoded channel-frame intermediates; same layout as oracle/lc3_oracle.h: lc3o_dec_trace */
typedef struct {
    int bfi, bw_idx, lastnz, lsb_mode, gg_idx, fac_ns, nfilt, tns_order[2], tns_idx[16], scf_idx[7], ltpf[3], nf_seed, zero_frame, nres;
    int xq[960]; float scf_q[16]; float q_gain[960]; float q_tns[960]; float q_shaped[960]; float x_imdct[960]; float x_out[960];
} lc3d_dec_trace;


/* stream lifecycle (include/lc3plus_batch.h: lc3plus_{enc,dec}_batch_{reset,export,import}_streams).  A stream's blob is LC3D_SS_HEADER bytes of header
 * (lc3_host.c stream_header), then its state rows, channel 0 first. */
#define LC3D_SS_HEADER 16
enum { LC3D_SS_RESET = 0, LC3D_SS_EXPORT = 1, LC3D_SS_IMPORT = 2 };

#ifdef __cplusplus
extern "C" {
#endif
/* tmpl: one channel-stream's fresh state row (DST_WORDS words, dec_init_state in lc3_host.c): kept on the device, every row starts from it */
int   lc3hip_dec_create(void** ctx, const lc3d_plan* plan, const float* tmpl, int n_streams, int device);
int   lc3hip_dec_upload_chans(void* ctx, const lc3d_dchan* chans, int first, int count);
int   lc3hip_dec_upload_table(void* ctx, const lc3d_dchan* tab, int n);      /* configuration per channel byte count 0 .. n - 1 (per-frame sizes) */
/* sizes_host: null, or [n_streams][n_frames] stream-frame sizes, 0 where lost (bfi_flags_host then holds every lost frame); sizes_max_nbytes: the largest
 * channel frame of the call that is not lost */
int   lc3hip_dec_decode(void* ctx, const void* frames, int frames_on_device, int in_stride, const uint8_t* bfi_flags_host, const uint16_t* sizes_host,
                        int sizes_max_nbytes, int n_frames, void* pcm, int pcm_on_device, int bps, uint8_t* status_host, void* hip_stream, int sync,
                        void* trace_host);
/* per-frame sizes (and bfi_dev, status_dev: null or) in device memory, as frames and pcm: ordered on hip_stream, does not wait unless sync; the per-stream
 * configuration on the device follows each stream's last good frame, the host's copy of it is then unknown (lc3hip_dec_download_chans) */
int   lc3hip_dec_decode_dsizes(void* ctx, const void* frames, int in_stride, const int32_t* num_bytes_dev, const uint8_t* bfi_dev, int n_frames,
                               void* pcm, int bps, uint8_t* status_dev, void* hip_stream, int sync);
/* the same with frames packed: frame (s, t) at frames + offsets_dev[s][t], the rule of lc3d_dec_frame_class_packed (capacity, max_bytes) */
int   lc3hip_dec_decode_packed(void* ctx, const void* frames, long long capacity, const long long* offsets_dev, const int32_t* num_bytes_dev, int max_bytes,
                               const uint8_t* bfi_dev, int n_frames, void* pcm, int bps, uint8_t* status_dev, void* hip_stream, int sync);
int   lc3hip_dec_download_chans(void* ctx, lc3d_dchan* chans);    /* waits for the last call, copies the per-channel-stream configuration to chans[ncs] */
float lc3hip_dec_last_ms(void* ctx);
/* what the frame probe borrows of a decoder context (lc3_probe_shim.h): its device, the plan and the per-size channel table in device memory - both written once, at
 * creation - and the context's stream.  Touches nothing. */
int   lc3hip_dec_probe_args(void* ctx, int* device, const lc3d_plan** plan_dev, const lc3d_dchan** tab_dev, int* tab_n, void** stream);
int   lc3hip_dec_destroy(void* ctx);
/* what the packet egress borrows of an encoder context (lc3_egress_shim.h): its device and, with want_stream, the context's own stream (created here where no
 * call has needed it yet).  Touches nothing else. */
int   lc3hip_stream_args(void* ctx, int want_stream, int* device, void** stream);
int   lc3hip_create(void** ctx, const lc3d_plan* plan, int n_streams, int device);
int   lc3hip_set_template(void* ctx, const float* tmpl);       /* one channel-stream's fresh state row (init_state): kept on the device, every row reset from it */
int   lc3hip_upload_chans(void* ctx, const lc3d_chan* chans, int first, int count);
/* the same, queued on hip_stream (NULL: the context's stream) behind the work already there, without waiting for it; later calls wait for the copy.
 * bw_only: the copy changes the bandwidth words alone (a following per-frame-bandwidth call may still overlap the call before it) */
int   lc3hip_upload_chans_async(void* ctx, const lc3d_chan* chans, int first, int count, void* hip_stream, int bw_only);
int   lc3hip_upload_enc_table(void* ctx, const lc3d_chan* tab, int n);   /* encoder configuration per channel byte count 0 .. n - 1 (per-frame bitrates) */
/* fsz_host: null, or [n_streams][n_frames] bytes of every stream-frame (per-frame bitrates; the host has checked them against the table).
 * bw_host: null, or [n_streams][n_frames] the bandwidth in force of every stream-frame in Hz (per-frame bandwidths; resolved and checked by the host,
 * standard layout only); the call takes the path it takes without it */
int   lc3hip_encode(void* ctx, const void* pcm, int pcm_on_device, int bitdepth, int n_frames, void* out, int out_stride,
                    int out_on_device, void* hip_stream, int sync, void* trace_host, const uint16_t* fsz_host, const uint16_t* bw_host);
/* per-frame rates_dev and / or bws_dev ([n_streams][n_frames] or null, not both) in device memory, as pcm and out: the rule of lc3d_enc_frame_step on the
 * device from each stream's carry, num_bytes_dev / flags_dev (null or [n_streams][n_frames]) written there; ordered on hip_stream, does not wait unless sync.
 * Each stream ends configured on the device with its carry; the host's copy of the configuration is then unknown (lc3hip_download_chans).  clear_resets: the
 * configuration holds pending one-shot attack-detector resets, which the call consumes */
int   lc3hip_encode_rates_device(void* ctx, const void* pcm, int bitdepth, int n_frames, void* out, int out_stride, const int32_t* rates_dev,
                                 const int32_t* bws_dev, const lc3d_rate_rule* rule, int32_t* num_bytes_dev, uint8_t* flags_dev, int clear_resets,
                                 void* hip_stream, int sync);
/* packed output (lc3plus_enc_batch_encode_packed): the call of lc3hip_encode_rates_device (rates_dev or bws_dev given) or of lc3hip_encode with device pointers
 * (neither), each frame written at its offset of an exclusive scan of the frame sizes in `order` (LC3D_PACK_*) where it fits capacity; offsets_dev, total_dev
 * (null or device) receive the scan, flags_dev bit LC3D_ENC_FL_PACK_CAP the frames that do not fit */
int   lc3hip_encode_packed(void* ctx, const void* pcm, int bitdepth, int n_frames, const int32_t* rates_dev, const int32_t* bws_dev, const lc3d_rate_rule* rule,
                           int order, void* out, long long capacity, long long* offsets_dev, long long* total_dev, int32_t* num_bytes_dev, uint8_t* flags_dev,
                           int clear_resets, void* hip_stream, int sync);
int   lc3hip_download_chans(void* ctx, lc3d_chan* chans);       /* waits for the last call, copies the per-channel-stream configuration to chans[ncs] */
float lc3hip_last_ms(void* ctx);
size_t lc3hip_state_bytes(void* ctx);                            /* checkpoint / resume of the per-stream state (include/lc3plus_batch.h) */
int   lc3hip_get_state(void* ctx, void* host, size_t bytes);
int   lc3hip_set_state(void* ctx, const void* host, size_t bytes);
size_t lc3hip_dec_state_bytes(void* ctx);
int   lc3hip_dec_get_state(void* ctx, void* host, size_t bytes);
int   lc3hip_dec_set_state(void* ctx, const void* host, size_t bytes);
/* One stream-lifecycle call, mode LC3D_SS_*, queued on hip_stream (NULL: the context's stream) behind every earlier call of the batch, whose later calls follow
 * it; the next call does not take the overlapped path (encoder: ahead_ok, decoder: parse-ahead).  streams [n]: host, checked by the caller.  cfg (reset): null,
 * or [n][channels] configuration entries written for the listed streams.  blob (export, import): n blobs, in host memory (staged through pinned memory; an
 * export returns with the data) or, with blob_on_device, in device memory (16-byte aligned).  hdr: the batch's 4-word blob header; an import writes a
 * stream only where its blob carries it, status (device import only, null or device [n]): 1 where it did not.  Waits for the device only with sync, for a
 * host export, and for the staging slot of the call LC3D_SETS back. */
int   lc3hip_stream_state(void* ctx, int mode, const int* streams, int n, const lc3d_chan* cfg, void* blob, int blob_on_device, const uint32_t* hdr,
                          uint8_t* status, void* hip_stream, int sync);
int   lc3hip_dec_stream_state(void* ctx, int mode, const int* streams, int n, const lc3d_dchan* cfg, void* blob, int blob_on_device, const uint32_t* hdr,
                              uint8_t* status, void* hip_stream, int sync);
/* placed PCM (include/lc3plus_batch.h: lc3plus_{enc,dec}_batch_set_pcm_placement; lc3_plan.h: lc3d_pcm_placed_*): offsets_dev [n_streams][n_frames of each call] in
 * device memory, or null: off; capacity in elements.  Kept in the context and read by every later call that takes device PCM - those calls refuse host PCM, traces
 * and the channel-major layout while it is on.  Queues nothing, waits for nothing. */
int   lc3hip_set_pcm_placement(void* ctx, const long long* offsets_dev, long long capacity);
int   lc3hip_dec_set_pcm_placement(void* ctx, const long long* offsets_dev, long long capacity);
/* per-stream frame counts (include/lc3plus_batch.h: lc3plus_dec_batch_set_frame_counts; lc3_plan.h: lc3d_dec_count_clamp): counts_dev [n_streams] in device memory,
 * or null: off.  Kept in the context; read on the device by lc3hip_dec_decode_dsizes and lc3hip_dec_decode_packed, which then launch the ragged kernels;
 * lc3hip_dec_decode fails while it is on (the host refuses first).  Queues nothing, waits for nothing. */
int   lc3hip_dec_set_frame_counts(void* ctx, const int32_t* counts_dev);
/* the encoder's counterpart (lc3plus_enc_batch_set_frame_counts; lc3_plan.h: LC3D_ENC_FL_ABSENT): read on the device by lc3hip_encode_rates_device and
 * lc3hip_encode_packed (rates_dev and bws_dev may then both be null), which launch the ragged kernels on the one-wave path; lc3hip_encode fails while it is on (the
 * host refuses first).  Queues nothing, waits for nothing. */
int   lc3hip_set_frame_counts(void* ctx, const int32_t* counts_dev);
int   lc3hip_dec_set_input_ready(void* ctx, int ready);          /* see lc3plus_dec_batch_set_input_ready (include/lc3plus_batch.h) */
int   lc3hip_set_input_ready(void* ctx, int ready);              /* see lc3plus_enc_batch_set_input_ready (include/lc3plus_batch.h) */
int   lc3hip_last_status(void* ctx, uint8_t* status_host, int n);        /* LC3D_ENC_ST_* bits per channel-frame of the last call; returns the count copied */
int   lc3hip_last_records(void* ctx, float* rec_host, int max_words);   /* the per-frame records of the last pipelined call [channel-stream][frame][FR_WORDS]; returns the words copied (0: the last call did not take that path) */
int   lc3hip_wait(void* ctx);                                      /* waits for the batch's last call (sync = 0 calls of a sharded batch) */
int   lc3hip_dec_wait(void* ctx);
int   lc3hip_destroy(void* ctx);
int   lc3hip_test_fastmath(int kind, const float* x_host, float* y_host, long long n);   /* test hook: the device's math over an array (0 log2, 1 log10, 2 2^x through lc3_fastmath.h; 3 pow(2, x), 4 pow(x, i mod 9) through the device library) */
/* The launch census: which kernel entry points this process has launched through lc3_runtime.hip, and how often.  Process-wide, off by default (a launch then reads
 * one flag); safe from several host threads.  enable: on != 0 counts from now on; reset: every count to 0; read: the launched kernels as "name count" lines (name: the
 * kernel's symbol in the code object) into buf, at most cap bytes with the terminating 0, and returns the bytes the whole text needs.  LC3PLUS_LAUNCH_CENSUS=<path>,
 * read once when the library is loaded, enables it and appends the same lines to <path> when the library is unloaded or the process exits. */
void  lc3hip_launch_census_enable(int on);
void  lc3hip_launch_census_reset(void);
size_t lc3hip_launch_census_read(char* buf, size_t cap);
/* Poisoned workspaces (DESIGN.md "Every workspace word"), a debugging aid read with the other LC3PLUS_* switches when a batch is created.  The work buffers of a
 * batch are the device buffers a call fills and reads itself, none of which a later call may rely on: the runtime lists them in one table per side.
 * LC3PLUS_POISON_WORK=A|B fills each of them with poison by element type where it is allocated (float 0xFFFFFFFF | 1.5f, int32 -1 | 1, uint16 and uint8 all ones | 1,
 * int64 -1 | -1); LC3PLUS_POISON_CALLS=1 (with the first) fills all of them again at the entry of every encode and decode call, between two waits for the device.
 * The two entries below walk the same table: buffer i of the batch - its member name (index in brackets where the member is an array), its device pointer (null
 * until a call has needed it), its length in bytes and its element type (LC3HIP_ELEM_*); they return 0, or 1 past the table's end.  Nothing is queued or waited
 * for: the caller waits for the batch first. */
enum { LC3HIP_ELEM_F32 = 1, LC3HIP_ELEM_I32 = 2, LC3HIP_ELEM_U16 = 3, LC3HIP_ELEM_U8 = 4, LC3HIP_ELEM_I64 = 5 };
int   lc3hip_work_buffer(void* ctx, int i, const char** name, void** ptr, size_t* bytes, int* elem);
int   lc3hip_dec_work_buffer(void* ctx, int i, const char** name, void** ptr, size_t* bytes, int* elem);
#ifdef __cplusplus
}
#endif
#endif
