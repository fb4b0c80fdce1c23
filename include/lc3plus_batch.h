/* lc3plus_batch.h -- batched multi-stream extension of the lc3_enc_* ABI (new in this engine).
 *
 * The reference encodes one frame of one stream per call (R/lc3.c:226-234 -> R/enc_lc3_fl.c:162-174).
 * Frames of ONE stream are not independent (MDCT overlap, pitch / LTPF memories and the rate-control
 * loop persist, R/setup_enc_lc3.h:17-62), but streams (and channels, R/enc_lc3_fl.c:167-171) are.
 * A batch therefore is n_streams independent encoder instances with identical (samplerate, frame_ms,
 * hrmode, channels) and a per-stream bitrate; each encode() call advances every stream by n_frames
 * frames with the per-stream state resident in HBM between calls.  One wavefront encodes one
 * channel-stream.  Plain pointers and sizes only.
 */
#ifndef LC3PLUS_BATCH_H
#define LC3PLUS_BATCH_H
#include "lc3.h"
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lc3plus_batch lc3plus_batch;

/* Creates n_streams encoders on HIP device `device` (-1 = current).  bitrates[n_streams] is the total
 * bitrate per stream (all channels), validated like lc3_enc_set_bitrate.  Error codes as lc3_enc_*. */
LC3_Error lc3plus_enc_batch_create(lc3plus_batch** batch, int n_streams, int samplerate, int channels,
                                   float frame_ms, int hrmode, const int* bitrates, int device);
LC3_Error lc3plus_enc_batch_destroy(lc3plus_batch* batch);

int lc3plus_enc_batch_input_samples(const lc3plus_batch* batch);    /* samples per channel per frame */
int lc3plus_enc_batch_num_bytes(const lc3plus_batch* batch, int stream); /* bytes per frame of that stream */
int lc3plus_enc_batch_stride(const lc3plus_batch* batch);           /* max over streams of num_bytes */
LC3_Error lc3plus_enc_batch_set_bitrate(lc3plus_batch* batch, int stream, int bitrate);
LC3_Error lc3plus_enc_batch_set_bandwidth(lc3plus_batch* batch, int stream, int bandwidth);

/* ---- The PCM format word ------------------------------------------------------------------------------------------------------------------
 * The `bitdepth` argument of every batched encode call and the `bps` argument of every batched decode call is a format word: a sample type, alone or
 * combined (|) with ONE layout.  16, 24 and 32 alone are what they always were.  Any other value is LC3_ERROR before any work is done.
 *
 * Sample type:
 *   16, 24, 32          : int16_t / int32_t as the reference takes and gives them (lc3_enc_fl bitdepth, lc3_dec_fl bps)
 *   LC3PLUS_PCM_FLOAT32 : IEEE float, full scale 1.0.  Encoder: the internal sample is x * 32768.0f and nothing else - no rounding and no clipping
 *                         (the integer formats do not clip either), so float input that lies on the 16-, 24- or 32-bit grid gives the bytes of that
 *                         integer format.  A NaN or an infinity is taken as 0.0f, so that one bad sample cannot stay in a stream's filter
 *                         memories for ever.  Decoder: the synthesised sample times 2^-15, neither rounded nor clipped (the integer formats round that
 *                         same value, R/dec_lc3_fl.c:115-127), so it may exceed [-1, 1).
 *   Five wire types, each an element of 1, 2 or 3 bytes that stands for one of the integer depths.  Encoder: the element becomes that integer and is then
 *   converted as that depth is, so a call in a wire type gives, byte for byte, what the same call gives for the converted int16_t / int32_t array.
 *   Decoder: the result of that depth for the same frame, then the step named here.  No alignment is required: any byte address is a valid pointer.
 *   LC3PLUS_PCM_S16_BE  : 2 bytes, big-endian (RTP L16), for 16: the bytes swapped.
 *   LC3PLUS_PCM_S24_3LE : 3 bytes, little-endian two's complement (the body of a 24-bit WAV file), for 24: sign-extended on the way in; on the way out
 *                         the 24-bit result saturated to [-8388608, 8388607] as R/tinywaveout_c.h:403-424 clips it (the int32_t format does not clip: a
 *                         sample it gives as INT32_MIN comes out as -8388608), then its low three bytes.
 *   LC3PLUS_PCM_S24_3BE : the same, big-endian (RTP L24, AES67).
 *   LC3PLUS_PCM_ULAW    : 1 byte, G.711 mu-law (PCMU), for 16.  Code c -> sample: k = ~c & 0xff, e = (k >> 4) & 7, q = k & 15, magnitude
 *                         ((2q + 33) << (e + 2)) - 132, negative when bit 7 of c is clear.  Sample x -> code: s = x < 0, y = s ? ~x : x (one's complement:
 *                         -1 has magnitude 0), a = min((y >> 2) + 33, 8191), e = floor(log2 a) - 5, q = (a >> (e + 1)) & 15,
 *                         code (s ? 0 : 0x80) | (7 - e) << 4 | (15 - q).
 *   LC3PLUS_PCM_ALAW    : 1 byte, G.711 A-law (PCMA), for 16.  Code c -> sample: k = c ^ 0x55, e, q as above, magnitude (2q + 1) << 3 for e == 0, else
 *                         ((2q + 33) << (e - 1)) << 3, negative when bit 7 of k is clear.  Sample x -> code: s, y as above, m = y >> 4, c7 = m for m <= 15,
 *                         else e = floor(log2 m) - 3, c7 = e << 4 | ((m >> (e - 1)) & 15); code (c7 | (s ? 0 : 0x80)) ^ 0x55.
 *                         Both expansions are the ITU-T G.711 tables at 16 bits; every A-law code and every mu-law code but 0x7f (negative zero) round-trips.
 * Layout of one call's n_streams x n_frames x channels x samples elements (N = samples per frame, time = frame * N + sample):
 *   none                      : [stream][frame][channel][sample]
 *   LC3PLUS_PCM_INTERLEAVED   : [stream][time][channel]         - capture, WAV and RTP order
 *   LC3PLUS_PCM_CHANNEL_MAJOR : [stream][channel][time]         - the frame count of THIS call is part of the address
 * With one channel the three are the same addresses.  A layout changes addresses only, never a byte or a sample.
 * Every format works with host and with device pointers; the device-pointer calls are the fast ones (float samples one after the other are loaded and
 * stored 16 bytes per lane like the 16-bit ones; interleaved samples one by one).  With host pointers, the channel-major layout is copied in one piece
 * instead of in overlapped runs of frames.  The traced calls (*_traced) take 16, 24 and 32 alone.
 * lc3plus_pcm_format_check and lc3plus_pcm_offset are host-only: the check every call makes, and the element index of one sample (-1 for arguments
 * out of range) - the arithmetic the kernels use.  The byte address of an element is its index times lc3plus_pcm_elem_bytes(format): 1, 2, 3 or 4, -1 for a
 * word the check refuses.  lc3plus_pcm_to_native converts n elements of a wire type to the int16_t / int32_t it stands for, lc3plus_pcm_from_native applies the
 * decoder's output step (saturation included) to n int16_t / int32_t: the rule above on the host, no device needed.  A layout bit in `format` is ignored; a type
 * that is not one of the five is LC3_ERROR, a null pointer LC3_NULL_ERROR. */
#define LC3PLUS_PCM_FLOAT32       0x80
#define LC3PLUS_PCM_S16_BE        0x81
#define LC3PLUS_PCM_S24_3LE       0x82
#define LC3PLUS_PCM_S24_3BE       0x83
#define LC3PLUS_PCM_ULAW          0x84
#define LC3PLUS_PCM_ALAW          0x85
#define LC3PLUS_PCM_INTERLEAVED   0x100
#define LC3PLUS_PCM_CHANNEL_MAJOR 0x200
LC3_Error lc3plus_pcm_format_check(int format);
int64_t lc3plus_pcm_offset(int format, int channels, int n_frames, int samples, int stream, int frame, int channel, int sample);
int lc3plus_pcm_elem_bytes(int format);
LC3_Error lc3plus_pcm_to_native(int format, const void* src, int64_t n, void* dst);
LC3_Error lc3plus_pcm_from_native(int format, const void* src, int64_t n, void* dst);

/* ---- Placed PCM: every frame of a call at an offset read from device memory (per-session rings, simulcast) ----
 * lc3plus_enc_batch_set_pcm_placement / lc3plus_dec_batch_set_pcm_placement (below, with the batches) make the PLACEMENT of the PCM free as the format word makes its
 * element free: frame (s, t) of a call lies where offsets[s * n_frames + t] says, so that an encoder reads straight out of capture rings, a decoder writes
 * straight into playout rings, and several streams encode one signal at several rates without a copy.
 *   offsets  : device pointer to int64 [n_streams][n_frames], indexed [s * n_frames + t] with the n_frames of each call.  NULL switches placement off: off is the
 *              default, and every call then behaves as without it.
 *   capacity : the length of the PCM buffer in elements, >= 0.
 * The setter only records the pair; it queues nothing and waits for nothing.  LC3_NULL_ERROR for a null batch, LC3_ERROR for capacity < 0.  Placement is
 * configuration, not state: get_state, set_state and the stream blobs do not carry it.
 * It applies to every later call of the batch that takes its PCM through a device pointer - encode / decode with *_on_device = 1, encode_bitrates /
 * encode_bandwidths with device PCM, encode_rates_device, encode_packed, decode_sizes, decode_sizes_device, decode_packed - and to the shards of a sharded batch
 * through the handle lc3plus_{enc,dec}_sharded_shard returns.  The array is read on the device when the call's kernels run: a kernel of the caller's may advance
 * ring positions between calls.  The set_input_ready promise covers `offsets` as it covers the PCM.
 * The address rule: offsets[s][t] is the element index, in the `pcm` argument of the call, of sample 0 of channel 0 of frame (s, t).  With no layout bit channel c
 * starts c * N elements further and its samples follow each other; with LC3PLUS_PCM_INTERLEAVED sample i of channel c is at + i * channels + c.  Either way a
 * frame occupies channels * N consecutive elements.  lc3plus_pcm_placed_offset is this arithmetic on the host: the element index of one sample, or -1 for
 * arguments out of range, a refused format word, or LC3PLUS_PCM_CHANNEL_MAJOR.  Every sample type of the format word works; the byte address is the index times
 * lc3plus_pcm_elem_bytes, and no alignment is needed beyond what the dense call of that type needs for its pointer.  Any element offset is exact; frames whose
 * byte address is a multiple of 16 keep the wide loads and stores.
 * While placement is on, a call with host PCM, a traced call, and a call with LC3PLUS_PCM_CHANNEL_MAJOR (its channel distance is a property of a dense call)
 * return LC3_ERROR, queue nothing and leave the batch unchanged.
 * A frame is VALID when 0 <= offset and offset + channels * N <= capacity, computed without overflow; lc3plus_plan_placed is that rule on the host (invalid[i] = 1
 * where offsets[i] is not valid; LC3_ERROR for a negative n or capacity, channels or samples below 1, a refused format word or channel-major, LC3_NULL_ERROR for
 * a null array with n > 0).  The host cannot see the offsets, so an invalid one does not fail the call, and memory outside [0, capacity) is never touched:
 *   encoder : all samples of an invalid frame are 0 wherever they are read - as the previous frame of the MDCT overlap, the resampler history and the attack
 *             detector as well.  The frame is encoded and its stream advances: the result equals a dense call in which that frame is silence.  The calls that
 *             return `flags` in device memory (encode_rates_device, encode_packed) set flag bit 4 (16) for it; the other calls stay silent.
 *   decoder : an invalid frame is decoded or concealed and its stream advances exactly as otherwise; its PCM is not written.  The calls with a device `status`
 *             (decode_sizes_device, decode_packed) set status bit 2 (4) for it; host status arrays keep their 0 / 1 meaning.
 * Input frames may coincide or overlap: several streams may read the same PCM (simulcast), and the hop may be shorter than a frame.  Output frames that overlap
 * are the caller's error: each is written whole, in no defined order.  No byte outside a written frame's channels * N elements is modified. */
int64_t lc3plus_pcm_placed_offset(int format, int channels, int samples, int64_t frame_offset, int channel, int sample);
LC3_Error lc3plus_plan_placed(int format, int channels, int samples, const int64_t* offsets, int64_t n, int64_t capacity, uint8_t* invalid);

/* Advances every stream by n_frames.
 *   pcm : [n_streams][n_frames][channels][input_samples] samples, int16_t (bitdepth 16) or int32_t (24/32); or float and / or another layout, as the
 *         format word in `bitdepth` says (above)
 *   out : [n_streams][n_frames][out_stride] bytes; frame payload = num_bytes(stream) bytes, rest untouched
 *   *_on_device : 0 = host pointer, 1 = device pointer used in place.  With BOTH on the host the call is cut into runs of frames
 *                 whose H2D copy, kernels and D2H copy overlap on three HIP streams; pinned caller memory (hipHostMalloc /
 *                 hipHostRegister) is copied in place, pageable memory is staged through the batch's pinned buffers
 *   hip_stream  : hipStream_t to enqueue on (NULL = the batch's own stream); the call returns after the
 *                 work is complete when sync != 0, otherwise right after enqueueing.                  */
LC3_Error lc3plus_enc_batch_encode(lc3plus_batch* batch, const void* pcm, int pcm_on_device, int bitdepth,
                                   int n_frames, void* out, int out_stride, int out_on_device,
                                   void* hip_stream, int sync);

/* Per-frame bitrates, as the reference takes them (R/codec_exe.c:296-302: lc3_enc_set_bitrate before every frame of a switching file).  Arguments
 * as encode(), and
 *   bitrates  : host pointer, [n_streams][n_frames] total bitrate of each stream-frame (all channels); may be reused when the call returns
 *   num_bytes : host pointer or NULL, [n_streams][n_frames]: bytes written per stream-frame
 * Frame t of stream s is encoded byte for byte as the reference encodes it right after lc3_enc_set_bitrate(bitrates[s][t]): the frame's bytes
 * split over its channels, the bit budgets, gain offset and regularisation bits, LPC weighting, the LTPF enable and attack handling - a frame
 * whose rate disables attack handling clears the attack detector first (R/setup_enc_lc3.c:297-308), and a later frame whose rate enables it
 * starts from that cleared state.  Bandwidths stay per stream (set_bandwidth).  Rates equal to the stream's current one everywhere give the
 * output of encode().  Every rate is checked before any work, with the limits of set_bitrate for the geometry (high-resolution minimums,
 * 44.1 kHz scaling): a rate outside them returns LC3_BITRATE_ERROR, an out_stride below the call's largest stream-frame LC3_ERROR, and the
 * batch is left unchanged.  Each frame's payload starts at its slot of out; the bytes behind it are untouched.  After the call each stream is
 * configured with its last frame's rate (num_bytes(stream), stride(), and a following encode() continue from it); the rates stay
 * configuration, not state (get_state / set_state are unchanged).  Host or device pointers, sync 0 or 1 and hip_stream as for encode(); the
 * new configuration is queued on hip_stream behind the call's kernels, so a call with sync = 0 returns without waiting for them.  The frames run in the
 * one-wave-per-channel-stream kernel, whose writer is inside it: last_status reports the call, last_records returns 0 words after it. */
LC3_Error lc3plus_enc_batch_encode_bitrates(lc3plus_batch* batch, const void* pcm, int pcm_on_device, int bitdepth,
                                            const int* bitrates, int n_frames, void* out, int out_stride, int out_on_device,
                                            int* num_bytes, void* hip_stream, int sync);

/* Per-frame bandwidths, as the reference takes them (R/codec_exe.c:316-325: lc3_enc_set_bandwidth before every frame of a bandwidth switching file).
 * Arguments as encode_bitrates(), and
 *   bandwidths : host pointer, [n_streams][n_frames] bandwidth in Hz for each stream-frame; may be reused when the call returns
 *   bitrates   : NULL, or as for encode_bitrates()
 *   num_bytes  : host pointer or NULL, [n_streams][n_frames]; without bitrates every entry is num_bytes(stream)
 * Frame t of stream s is encoded byte for byte as the reference encodes it right after lc3_enc_set_bitrate(bitrates[s][t]) (when bitrates are given)
 * and then lc3_enc_set_bandwidth(bandwidths[s][t]): 0 switches the bandwidth controller off for the frame; a value set_bandwidth refuses
 * (2 * bw > min(samplerate, 40000), R/lc3.c:193-199) keeps the bandwidth in force - the call still does all its work and returns LC3_BW_WARNING
 * instead of LC3_OK.  Refused calls, checked in this order, queue nothing and leave the batch unchanged: a high-resolution batch
 * (LC3_HRMODE_BW_ERROR, as set_bandwidth); a negative bandwidth, or a positive one whose cut-off line bw * frame_ms / 500 is below 1 (under 50 Hz at
 * 10 ms, 100 Hz at 5 ms, 200 Hz at 2.5 ms): LC3_ERROR; NULL pointers, bitdepth and n_frames as encode(); a rate or out_stride as encode_bitrates().
 * After the call each stream is configured with the bandwidth in force after its last frame (bandwidth(stream)), and with its last rate when
 * bitrates were given; a following encode() continues from there.  Bandwidths stay configuration, not state: get_state / set_state and the stream
 * blobs are unchanged.  The new configuration is queued on hip_stream behind the call's kernels, so a call with sync = 0 does not wait for them.
 * Without bitrates the call takes the path encode() takes for the same n_frames, promise and switches - the pipelined kernels for longer calls, the
 * overlap of consecutive equal-length calls under set_input_ready - and last_records / last_status report it as they report encode() (FR_BWC holds
 * each frame's capped bandwidth index); with bitrates it runs the one-wave kernel of encode_bitrates().  The diagnostic switches LC3PLUS_ENC_FUSED,
 * LC3PLUS_ENC_NO_SPLIT and LC3PLUS_ENC_SHAPE_WAVE select the same kernels as for encode(), each in its per-frame-bandwidth form, with the same bytes. */
LC3_Error lc3plus_enc_batch_encode_bandwidths(lc3plus_batch* batch, const void* pcm, int pcm_on_device, int bitdepth,
                                              const int* bandwidths, const int* bitrates, int n_frames, void* out, int out_stride,
                                              int out_on_device, int* num_bytes, void* hip_stream, int sync);
int       lc3plus_enc_batch_bandwidth(const lc3plus_batch* batch, int stream);     /* Hz in force, 0 = none; -1 on a bad argument */
/* The per-frame rule of encode_bandwidths() on the host alone, no device: start [n_streams] the bandwidth in force before the call, bandwidths
 * [n_streams][n_frames] -> in_force [n_streams][n_frames].  Returns LC3_OK, LC3_BW_WARNING where a value was refused, or the call's error. */
LC3_Error lc3plus_enc_plan_bandwidths(int samplerate, float frame_ms, int hrmode, int n_streams, const int* start,
                                      const int* bandwidths, int n_frames, int* in_force);

/* Per-frame rates and bandwidths in device memory, for servers whose rate control runs on the GPU.  Every pointer is a device pointer:
 *   pcm        : [n_streams][n_frames][channels][input_samples], int16_t (bitdepth 16) or int32_t (24/32)
 *   bitrates   : [n_streams][n_frames] total bitrate of each stream-frame, or NULL
 *   bandwidths : [n_streams][n_frames] bandwidth in Hz of each stream-frame, or NULL (not both NULL)
 *   out        : [n_streams][n_frames][out_stride] bytes; each payload at its slot, the bytes behind it and every slot outside the call untouched
 *   num_bytes  : [n_streams][n_frames] bytes written per stream-frame, or NULL
 *   flags      : [n_streams][n_frames], or NULL: bit 0 the rate was refused, bit 1 the bandwidth was refused as set_bandwidth refuses it, bit 2 the
 *                bandwidth was negative or its cut-off line below 1; 0 for a clean frame
 * The call is queued on hip_stream (NULL = the batch's own stream) in order with the batch's other calls there, and returns at once when sync = 0: it
 * does not wait, copy synchronously or read anything back - except that a call with more frames than any earlier one, on a batch that already holds
 * smaller buffers, waits once for the device while it grows them.  Refused calls, checked in this order, queue nothing and leave the batch unchanged:
 * NULL pcm or out, or both bitrates and bandwidths NULL (LC3_NULL_ERROR); a bad bitdepth, n_frames <= 0, or out_stride below the stride bound (below)
 * (LC3_ERROR); bandwidths on a high-resolution batch (LC3_HRMODE_BW_ERROR); bandwidths while a stream's bandwidth in force, installed by set_bandwidth,
 * has a cut-off line below 1 (LC3_ERROR, as encode_bandwidths).  Frame t of stream s applies the rate and then the bandwidth, each with the rule of
 * encode_bitrates() / encode_bandwidths() and byte for byte as they encode every input they accept, on the device, from the stream's configuration
 * before the call and carried across frames and calls of every kind.  An entry they would refuse does not fail this call; the frame goes on as the
 * reference does after a refused setter: a rate outside the limits of set_bitrate, or whose stream-frame exceeds out_stride, encodes the frame at the
 * carried rate (flag bit 0); a bandwidth set_bandwidth refuses (bit 1), or out of range (bit 2), keeps the bandwidth in force.  The result is LC3_OK
 * even where frames were flagged; last_status reports the call as for encode_bitrates(), last_records as for encode_bandwidths() without rates.
 * With bitrates the call runs the kernels of encode_bitrates(); with bandwidths alone it takes the path of encode_bandwidths(), including the overlap
 * of consecutive calls under set_input_ready, whose promise covers bitrates and bandwidths as it covers the PCM.
 * After the call each stream is configured on the device with its last valid rate and its last bandwidth in force.  The first host-side reader or writer
 * of the configuration (num_bytes, stride, bandwidth, set_bitrate, set_bandwidth, encode_bitrates, encode_bandwidths, reset_streams with rates) waits
 * for the batch's last call and reads it back, once.  encode() and this call do not: they check out_stride against a stride bound, which is stride()
 * while the host's copy is current and is raised to the out_stride of every call of this kind with bitrates; a caller who wants a smaller out_stride
 * calls stride() first.  Rates and bandwidths stay configuration, not state: get_state / set_state and the stream blobs are unchanged. */
LC3_Error lc3plus_enc_batch_encode_rates_device(lc3plus_batch* batch, const void* pcm, int bitdepth, const int32_t* bitrates,
                                                const int32_t* bandwidths, int n_frames, void* out, int out_stride, int32_t* num_bytes,
                                                uint8_t* flags, void* hip_stream, int sync);
/* The per-frame rule of encode_rates_device() on the host alone, no device: start_rates, start_bw [n_streams] the configuration before the call,
 * bitrates, bandwidths NULL or [n_streams][n_frames] -> num_bytes, bw_in_force, flags [n_streams][n_frames] and end_rates [n_streams].  Returns the
 * call's error for the arguments (a start rate that is not a valid one fitting out_stride: LC3_BITRATE_ERROR), LC3_OK otherwise. */
LC3_Error lc3plus_enc_plan_rates_lenient(int samplerate, int channels, float frame_ms, int hrmode, int n_streams, const int* start_rates,
                                         const int* start_bw, const int* bitrates, const int* bandwidths, int n_frames, int out_stride,
                                         int* num_bytes, int* bw_in_force, uint8_t* flags, int* end_rates);

/* Packed output in device memory, for senders that want their packets back to back (an RTP-style ring) without compacting fixed slots themselves.
 * Every pointer is a device pointer:
 *   pcm, bitrates, bandwidths : as encode_rates_device(), except that bitrates and bandwidths may both be NULL (fixed per-stream rates, as encode())
 *   order        : LC3PLUS_PACK_STREAM_MAJOR (stream 0 frames 0 ... n_frames - 1, then stream 1, ...) or LC3PLUS_PACK_FRAME_MAJOR (frame 0 of streams 0 ...
 *                  n_streams - 1, then frame 1, ...): how the frames lie in out
 *   out          : out_capacity bytes; frame (s, t) is written to out + offsets[s * n_frames + t], exactly its num_bytes bytes long
 *   offsets      : [n_streams][n_frames] int64 (always indexed [s][t]), or NULL: an exclusive scan of the frame sizes in `order`, starting at 0
 *   total        : one int64, or NULL: the sum of all frame sizes of the call
 *   num_bytes, flags : as encode_rates_device(), and flag bit 3 (8): the frame did not fit out_capacity (offset + size > out_capacity)
 * Frame t of stream s is encoded as encode_rates_device() encodes it (as encode() without bitrates and bandwidths), with its per-frame rule and the carry across
 * calls of every kind - except that there is no out_stride: a rate is refused (flag bit 0) only where set_bitrate refuses it.  A frame that does not fit
 * out_capacity is still encoded and its stream advances; its bytes are not written.  No byte of out outside [offset, offset + size) of a written frame is
 * touched, bytes at or past out_capacity included.  Refused calls queue nothing and leave the batch unchanged: NULL pcm or out (LC3_NULL_ERROR); a bad
 * bitdepth, n_frames <= 0, an order other than 0 / 1, or out_capacity < 0 (LC3_ERROR); then the refusals of encode_rates_device() for bandwidths.  Queueing,
 * sync = 0, buffer growth, the configuration left on the device and the set_input_ready promise are those of encode_rates_device() (of encode() without
 * bitrates and bandwidths); the promise covers offsets and total as it covers the output buffer.  The call takes the kernel path encode_rates_device() (or
 * encode()) takes for the same arguments - the one-wave kernel with its writer inside, the pipelined writer, the large layout, the diagnostic switches - each
 * in a packed form, behind one scan of the call's frame sizes (three short kernels on the stream of the call's sizes).  The diagnostic large-frame writer
 * (a frame per wave, off by default) has no packed form: a packed call uses the one-frame-per-lane writer there. */
#define LC3PLUS_PACK_STREAM_MAJOR 0
#define LC3PLUS_PACK_FRAME_MAJOR  1
LC3_Error lc3plus_enc_batch_encode_packed(lc3plus_batch* batch, const void* pcm, int bitdepth, const int32_t* bitrates, const int32_t* bandwidths, int n_frames,
                                          int order, void* out, int64_t out_capacity, int64_t* offsets, int64_t* total, int32_t* num_bytes, uint8_t* flags,
                                          void* hip_stream, int sync);
/* The offsets of encode_packed() on the host alone, no device: sizes [n_streams][n_frames] -> offsets [n_streams][n_frames] (indexed [s][t]), *total (or NULL)
 * the sum, overflow (or NULL) [n_streams][n_frames] 8 where offset + size > capacity, 0 elsewhere.  LC3_ERROR for n_streams or n_frames <= 0, a bad order
 * or capacity < 0. */
LC3_Error lc3plus_plan_packed(const int32_t* sizes, int n_streams, int n_frames, int order, int64_t capacity, int64_t* offsets, int64_t* total,
                              uint8_t* overflow);

/* Checkpoint / resume.  The cross-frame state of every channel-stream of the batch (MDCT / resampler memory, pitch and LTPF histories,
 * rate-control and attack-detector words; R/setup_enc_lc3.h:17-62) as one opaque host array of state_size() bytes.  A batch created with
 * the same (n_streams, samplerate, channels, frame_ms, hrmode, bitrates, bandwidths) that is given the state continues the streams
 * exactly where the first one stopped - on another GPU or in another process.  Both calls wait for the last encode() to finish. */
size_t    lc3plus_enc_batch_state_size(const lc3plus_batch* batch);
LC3_Error lc3plus_enc_batch_get_state(lc3plus_batch* batch, void* state, size_t size);
LC3_Error lc3plus_enc_batch_set_state(lc3plus_batch* batch, const void* state, size_t size);

/* Stream lifecycle: reset, export and import single streams of a batch, without touching the others.  A server starts a session in a free slot with
 * reset_streams, and moves a live stream to another batch or device with export_streams / import_streams.
 *   streams    : host array of n stream indices, each in [0, n_streams) and none twice; may be reused when the call returns.  NULL (streams, blob):
 *                LC3_NULL_ERROR; n <= 0, an index out of range or repeated: LC3_ERROR.  Every argument is checked before any work: on an error nothing is queued.
 *   hip_stream : the call is queued there (NULL = the batch's own stream) behind every earlier call of the batch - pipelined calls whose work is still on
 *                the batch's side streams included - and every later call sees the state it leaves.  With sync = 0 it returns after queueing: it does not wait
 *                for the device, copy synchronously or read anything back, except an export into a host blob, which returns with the data.  The call after
 *                a reset or import runs ordered (the encoder's pipelined call does not take the MDCT memory from the previous call's hand-over, the decoder's
 *                parse-ahead waits); results are byte-identical either way.
 * reset_streams: every listed stream's state becomes that of a freshly created stream (what lc3_enc_init gives).  bitrates: NULL keeps each stream's
 *                configuration; otherwise [n] total bitrates, each listed stream configured as set_bitrate configures it (bandwidth kept) - every rate is
 *                checked before any work, a bad one returns LC3_BITRATE_ERROR and changes nothing.
 * Blob         : stream_state_size() bytes per stream: a 16-byte header naming the codec (encoder / decoder), the geometry (sample rate, frame length, hrmode,
 *                channels) and the row length, then the stream's state rows, channel 0 first - exactly the bytes get_state() holds for that stream.  An
 *                export writes n blobs back to back, in list order.  blob_on_device: 0 = host memory, 1 = device memory, 16-byte aligned (LC3_ERROR otherwise).
 * import_streams: the blobs must come from a batch of the same codec and geometry; a stream's header is checked before its rows are written, and a
 *                mismatched stream is never written.  Host blob: every header is checked first, a mismatch returns LC3_ERROR and nothing is queued; the blob
 *                is staged through pinned memory and may be reused when the call returns; status (host [n] or NULL) is all 0.  Device blob: the kernel checks
 *                each header - status (device [n] or NULL) is 1 for a stream whose header does not match, which is left unchanged, 0 for the others.  Import
 *                does not change configuration: set the bitrate as after set_state. */
size_t    lc3plus_enc_batch_stream_state_size(const lc3plus_batch* batch);
LC3_Error lc3plus_enc_batch_reset_streams(lc3plus_batch* batch, const int* streams, int n, const int* bitrates, void* hip_stream, int sync);
LC3_Error lc3plus_enc_batch_export_streams(lc3plus_batch* batch, const int* streams, int n, void* blob, int blob_on_device, void* hip_stream, int sync);
LC3_Error lc3plus_enc_batch_import_streams(lc3plus_batch* batch, const int* streams, int n, const void* blob, int blob_on_device, uint8_t* status,
                                           void* hip_stream, int sync);

/* A promise about device-pointer calls, off by default: with ready != 0 the caller guarantees that the PCM passed to every following
 * encode() call is COMPLETE in device memory when the call is made - not merely queued earlier on hip_stream (so it is wrong for PCM
 * that a kernel or copy queued on hip_stream is still producing).  The batch then lets the frame-parallel and pitch kernels of a
 * call start on its own streams while the sequential tail and the bitstream writer of the previous call on the same hip_stream are
 * still running (consecutive calls of equal n_frames of up to 256 frames; up to three calls are then in flight); results are identical, and the output of a call is complete in stream order
 * on hip_stream as before.  The promise covers the OUTPUT buffer as well: it must be free to be written when the call is made - not still being read by work
 * queued earlier on hip_stream - because the bitstream writers of consecutive calls may run beside each other (large frames, short calls), each into the
 * buffer of its own call.  Streaming servers that fill their PCM ring ahead of the encode calls and drain their output ring behind them are the use.
 * For encode_rates_device() the promise covers its bitrates and bandwidths as well (complete when the call is made), and its num_bytes and flags as
 * the output buffer (free to be written). */
LC3_Error lc3plus_enc_batch_set_input_ready(lc3plus_batch* batch, int ready);
/* Placed PCM for the encoder's input ("Placed PCM" above): offsets NULL = off. */
LC3_Error lc3plus_enc_batch_set_pcm_placement(lc3plus_batch* batch, const int64_t* offsets, int64_t capacity);
/* Per-stream frame counts for the encoder (the counterpart of lc3plus_dec_batch_set_frame_counts below: a transcoder that decoded a jittery tick raggedly has PCM
 * for three frames of one stream, one of another and none of a third, and hands exactly that on).
 *   counts : device pointer to int32 [n_streams], or NULL = off (the default; every call then behaves as without this function)
 * The setter only records the pointer: it queues nothing and waits for nothing (LC3_NULL_ERROR for a NULL batch).  Counts are configuration, not state:
 * get_state / set_state and the stream blobs do not carry them.  Through lc3plus_enc_sharded_shard() they apply to that shard, with its local stream indices.
 * While counts are set they apply to encode_rates_device() and encode_packed(), the calls that return num_bytes / flags in device memory; the array is read on
 * the device when the call's kernels run, so a kernel or copy queued earlier on the same hip_stream may produce it - the decoder batch's counts array can be
 * handed over as it is.  A ragged call is ordered on hip_stream like a stream-lifecycle call: it does not overlap the previous call under set_input_ready(),
 * and the call after it runs ordered too.  Every other encode call of the batch - encode(), encode_bitrates(), encode_bandwidths(), the traced calls -
 * returns LC3_ERROR, queues nothing and leaves the batch unchanged; lc3plus_enc_sharded_encode() and _encode_device() make that check for all shards before
 * any shard is touched.
 *
 * The rule.  With c = min(max(counts[s], 0), n_frames) for a call of n_frames, of stream s
 *   frames t < c are PRESENT: exactly as in the same call without counts - the lenient rate / bandwidth rule with its carry and flag bits 0 ... 2, placed PCM
 *     with flag bit 4, packed output with flag bit 3, every PCM format word and layout (LC3PLUS_PCM_CHANNEL_MAJOR: the channel distance stays n_frames);
 *   frames t >= c are ABSENT: their bitrates, bandwidths and placement entries are not looked at - no result depends on their values, which may be left
 *     uninitialised; the arrays still hold n_frames entries per stream, and a kernel may load an absent entry with its neighbours (a group of four rates, a
 *     placement entry) without using it - no sample of their PCM is read, not as the "next" or "previous" frame of a present one either, they are not encoded, no byte of out is written for them, num_bytes[s][t] is 0, flags[s][t] is exactly 32
 *     (bit 5, "absent", LC3PLUS_ENC_FL_ABSENT, and no other bit) and their last_status entries are 0.
 * Packed output: an absent frame has size 0 in the scan - offsets[s][t] is the running offset at its place in `order`, total the sum over the present frames
 * (what lc3plus_plan_packed gives for sizes with zeros in them).
 * After the call the stream's state (MDCT overlap, pitch and LTPF histories, attack detector, rate loop) is the state after its c present frames, and its
 * configured rate and bandwidth those after its last present frame; with c = 0 state and configuration are bit for bit what they were - a one-shot
 * attack-detector reset pending from set_bitrate() included, which takes effect at the stream's first present frame, whenever that comes.  So a sequence of
 * ragged calls gives each stream the bytes, sizes and flags that one dense sequence of its present frames gives, and counts that all equal n_frames give the
 * bytes, sizes, flags and state of the call without counts.  ("State": every word a later frame reads.  get_state() also returns per-frame scalars that the
 * one-wave kernels store and the pipelined kernels leave alone, and unused words in front of the MDCT memory; counts that all equal n_frames give the
 * get_state() bytes of the dense call wherever both take the same path - which includes long calls without per-frame bitrates, see the last paragraph - and
 * where they do not, those bytes differ as they do between a short and a long dense call, and the batches carry on alike.)  Only a tail can be absent: a
 * count skips no frame in the middle of a call.
 * Changed with this function: lc3plus_enc_batch_set_bitrate() no longer drops a one-shot reset that is still pending.  A rate that disables attack handling
 * followed, with no frame of the stream between, by one that enables it now clears the detector, as the reference does at the disabling call
 * (setup_enc_lc3.c:297-308); before, the second call cancelled the first one's reset.
 * Which kernels carry a ragged call out.  It takes the pipelined path - a ragged form of every step, absent frames costing close to nothing - when all of
 * these hold: it has no per-frame bitrates (with them the dense call runs the one-wave kernel too); the batch uses the standard kernel layout (every operating
 * point but 96 kHz at 10 and 5 ms); n_frames > 8, with or without set_input_ready() - the lower threshold under the promise exists because calls overlap there,
 * and a ragged call does not; and none of the diagnostic kernel switches is set (LC3PLUS_ENC_FUSED, _NO_SPLIT, _SHAPE_WAVE, _SCF_WAVE, _PACK_SPLIT,
 * _TAILW_BYTES).  Every other ragged call runs one channel-stream per wavefront, the path of short calls: the large layout and the diagnostic writer variants
 * (head / code split, frame per wave) have no ragged forms.  LC3PLUS_ENC_RAGGED_PIPE=0, read when the batch is created, sends every ragged call down the
 * one-wave path: the results are the same.  last_status and last_records report a ragged pipelined call as they report a dense one; an absent frame's status
 * is 0, and the record words of an absent frame are unspecified. */
#define LC3PLUS_ENC_FL_ABSENT 32
LC3_Error lc3plus_enc_batch_set_frame_counts(lc3plus_batch* batch, const int32_t* counts);
/* That rule on the host alone, no device: lc3plus_enc_plan_rates_lenient with counts, host int32 [n_streams] or NULL = dense; bitrates and bandwidths may both
 * be NULL (encode_packed with neither).  Absent entries: num_bytes 0, bw_in_force 0, flags 32; end_rates is taken after the last present frame. */
LC3_Error lc3plus_enc_plan_rates_ragged(int samplerate, int channels, float frame_ms, int hrmode, int n_streams, const int* start_rates,
                                        const int* start_bw, const int* bitrates, const int* bandwidths, int n_frames, int out_stride,
                                        int* num_bytes, int* bw_in_force, uint8_t* flags, int* end_rates, const int32_t* counts);

/* Kernel-only timing of the last encode() call in milliseconds (HIP events on the launch stream). */
float lc3plus_enc_batch_last_kernel_ms(lc3plus_batch* batch);

/* Per channel-frame status of the last encode() call (device-pointer calls and host calls short enough for one run): conditions the
 * reference only asserts on - bit 0: side information + range-coder bits exceed the frame (R/ari_codec.c:777), bit 1: a quantised
 * line outside int16 outside the high-resolution mode (R/quantize_spec.c:50).  status: host array [n_streams * channels][n_frames];
 * returns the number of entries written (0 before the first call), negative on error.  Waits for the call to finish. */
int lc3plus_enc_batch_last_status(lc3plus_batch* batch, uint8_t* status, int max_entries);

/* Diagnostics: the per channel-frame records the kernels of the pipelined path hand to each other, of the last encode() call that took that path
 * (calls of more than 8 frames - more than 5 under the input-ready promise - that are neither traced nor run with LC3PLUS_ENC_FUSED / _NO_SPLIT, and the ragged
 * calls that take it, lc3plus_enc_batch_set_frame_counts above: the words of their absent frames are unspecified; 0 words when the last call did not take it): host array [n_streams * channels][n_frames][lc3plus_enc_batch_record_words()] of 32-bit words
 * - 16 scale factors, 16 quantised scale factors, 7 SNS indices, bandwidth index, attack-detector words, 4 LTPF words, 20 TNS words (filters,
 * orders, bits, coefficient indices), gain floor, all-zero flag, bandwidth behind the controller, and gain index / gain / bit count / last
 * non-zero line of the first quantisation (layout: FR_* in audio_codec_amd/csrc/lc3_plan.h).  The stage-level parity tests compare them with the
 * reference restatement's trace of the same frames.  Returns the words written, negative on error.  Waits for the call to finish. */
int lc3plus_enc_batch_last_records(lc3plus_batch* batch, float* records, int max_words);
int lc3plus_enc_batch_record_words(void);

/* Diagnostics: work buffer i of the batch - one of the device buffers a call fills and reads itself, as the host runtime lists them (the same list
 * LC3PLUS_POISON_WORK fills, INTEGRATION.md "Poisoned workspaces"): its name, its device pointer (null until a call has needed it), its length in bytes and
 * its element type (1 float32, 2 int32, 3 uint16, 4 uint8, 5 int64).  name is valid until the calling thread's next call of either function.  Returns LC3_OK,
 * or LC3_ERROR past the last buffer.  Waits for the batch's last call.  The tests read the buffers back through it (the decoder's: below). */
LC3_Error lc3plus_enc_batch_work_buffer(lc3plus_batch* batch, int i, const char** name, void** ptr, size_t* bytes, int* elem);

/* ---- batched decoder: n_streams independent decoder instances, one wavefront per channel-stream; same
 * conventions as the encoder batch.  num_bytes[n_streams] = bytes per stream-frame (all channels; may be NULL
 * and set later per stream, or come with the frames: lc3plus_dec_batch_decode_sizes, from host arrays, or
 * lc3plus_dec_batch_decode_sizes_device, from device memory).  R/dec_lc3_fl.c:134-163 is what one (stream, frame) does. ---- */
typedef struct lc3plus_dec_batch lc3plus_dec_batch;
LC3_Error lc3plus_dec_batch_create(lc3plus_dec_batch** batch, int n_streams, int samplerate, int channels,
                                   float frame_ms, int hrmode, const int* num_bytes, int device);
LC3_Error lc3plus_dec_batch_destroy(lc3plus_dec_batch* batch);
int       lc3plus_dec_batch_output_samples(const lc3plus_dec_batch* batch);
int       lc3plus_dec_batch_delay(const lc3plus_dec_batch* batch);
int       lc3plus_dec_batch_num_bytes(const lc3plus_dec_batch* batch, int stream);
LC3_Error lc3plus_dec_batch_set_num_bytes(lc3plus_dec_batch* batch, int stream, int num_bytes);
/*   frames : [n_streams][n_frames][in_stride] bytes (payload = num_bytes(stream) bytes at the start of each slot)
 *   bfi    : host pointer, [n_streams][n_frames] bad-frame flags (1 = conceal) or NULL
 *   pcm    : [n_streams][n_frames][channels][output_samples], int16_t (bps 16) or int32_t (24/32)
 *   status : host pointer or NULL, [n_streams][n_frames]: 1 where the frame was concealed (LC3_DECODE_ERROR) */
LC3_Error lc3plus_dec_batch_decode(lc3plus_dec_batch* batch, const void* frames, int frames_on_device, int in_stride,
                                   const uint8_t* bfi, int n_frames, void* pcm, int pcm_on_device, int bps,
                                   uint8_t* status, void* hip_stream, int sync);
/* Per-frame frame sizes, as the reference takes them (R/dec_lc3_fl.c:134-163: one size per lc3_dec_fl call).  Arguments as decode(), and
 *   num_bytes : host pointer, [n_streams][n_frames] bytes of each stream-frame (all channels); 0 = lost frame (R/dec_lc3_fl.c:140-143)
 *   bfi       : host pointer or NULL, [n_streams][n_frames] flags 0 or 1 (any other value: LC3_ERROR)
 * Per stream: a frame is lost where bfi is 1 or its size is 0, and is concealed (status 1).  A good frame configures its channels from its own size,
 * split over the channels as the reference does; a lost frame keeps the configuration of the stream's last good frame - across calls: the first
 * frame of a call carries the size the stream had before it (from create, set_num_bytes or the last good frame of an earlier call).  After the
 * call num_bytes(stream) is the size of the stream's last good frame, and a later decode() continues from it; the frame sizes stay configuration,
 * not state (get_state / set_state are unchanged: a checkpoint resumes on a batch created with those sizes).  A lost frame's slot is never read.
 * Every good size is checked before any work: outside the limits of the geometry, or larger than in_stride, the call returns LC3_NUMBYTES_ERROR
 * and decodes nothing (the reference fails at the bad frame, after decoding the ones before it).  The call is ordered and returns when it is done,
 * as a decode() with bfi; frames and pcm may be device pointers. */
LC3_Error lc3plus_dec_batch_decode_sizes(lc3plus_dec_batch* batch, const void* frames, int frames_on_device, int in_stride,
                                         const int* num_bytes, const uint8_t* bfi, int n_frames, void* pcm, int pcm_on_device,
                                         int bps, uint8_t* status, void* hip_stream, int sync);
/* Per-frame frame sizes and bad-frame flags in device memory, for receivers whose packets never reach the host.  Every pointer is a device pointer:
 *   frames    : [n_streams][n_frames][in_stride] bytes
 *   num_bytes : [n_streams][n_frames] bytes of each stream-frame (all channels); 0 = lost frame
 *   bfi       : [n_streams][n_frames] flags, or NULL
 *   pcm       : [n_streams][n_frames][channels][output_samples], int16_t (bps 16) or int32_t (24/32)
 *   status    : [n_streams][n_frames], or NULL: bit 0 the frame was concealed, bit 1 it was concealed because its size or flag was invalid
 *               (bit 2: placed PCM, the frame's offset is invalid; bit 3: the frame is absent, lc3plus_dec_batch_set_frame_counts below)
 * The call is queued on hip_stream (NULL = the batch's own stream) in order with the batch's other calls there, and returns at once when sync = 0: it
 * does not wait, copy synchronously or read anything back.  The arguments are checked on the host before any work - NULL frames, pcm or num_bytes:
 * LC3_NULL_ERROR; a bad bps, n_frames <= 0 or in_stride <= 0: LC3_ERROR; nothing is queued then.  The frame rule of decode_sizes() holds per stream,
 * evaluated on the device, with its carry across calls of both kinds - except that a size or flag decode_sizes() refuses does not fail this call: a
 * size outside the geometry's limits for any channel of the split, larger than in_stride or negative, or a flag other than 0 / 1, makes its frame lost
 * (concealed, status bit 1; it does not move the carry and its slot is never read).  After the call each stream is configured with its last good size
 * on the device; the first host-side reader after such calls (num_bytes, set_num_bytes, decode, decode_sizes) waits for the batch's last call and reads
 * that configuration back, once.  The parser stages frames in LDS up to ceil(in_stride / channels) bytes per channel (the host does not see the
 * sizes): a tight in_stride keeps the staged parser.  Consecutive calls with sync = 0 on different hip_streams are not ordered with each other.  A call
 * with more frames than any earlier call, on a batch that already holds smaller buffers, waits once for the device while it grows them. */
LC3_Error lc3plus_dec_batch_decode_sizes_device(lc3plus_dec_batch* batch, const void* frames, int in_stride, const int32_t* num_bytes,
                                                const uint8_t* bfi, int n_frames, void* pcm, int bps, uint8_t* status,
                                                void* hip_stream, int sync);
/* Frames packed back to back in device memory, for receivers whose packets land in a receive ring.  As decode_sizes_device(), with
 *   frames          : frames_capacity bytes; frame (s, t) is read from frames + offsets[s * n_frames + t], num_bytes[s][t] bytes
 *   offsets         : [n_streams][n_frames] int64 - any offsets: odd, out of order, with gaps (the offsets of encode_packed() fit directly)
 *   max_frame_bytes : the largest frame the call may hold (> 0)
 * The frame rule is decode_sizes_device()'s with in_stride replaced: a good frame also needs 0 <= offset, offset + size <= frames_capacity and size <=
 * max_frame_bytes.  A frame that breaks the rule is concealed with status bit 1, its bytes are never read and it does not move the carried size; a lost
 * frame's offset is not looked at.  Only the aligned words that hold a byte of a good frame are read.  The parser stages frames in LDS up to
 * ceil(max_frame_bytes / channels) bytes per channel: a tight max_frame_bytes keeps the staged parser.  Refused calls queue nothing: NULL frames, offsets,
 * num_bytes or pcm (LC3_NULL_ERROR); a bad bps, n_frames <= 0, max_frame_bytes <= 0 or frames_capacity < 0 (LC3_ERROR).  The call takes the path of
 * decode_sizes_device() and is queued and ordered the same way. */
LC3_Error lc3plus_dec_batch_decode_packed(lc3plus_dec_batch* batch, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes,
                                          int max_frame_bytes, const uint8_t* bfi, int n_frames, void* pcm, int bps, uint8_t* status, void* hip_stream, int sync);
/* The frame rule of decode_packed() on the host alone, no device: start [n_streams] the sizes before the call, num_bytes, offsets, bfi (or NULL)
 * [n_streams][n_frames] -> eff (the size in force), lost, invalid [n_streams][n_frames], end [n_streams] the sizes after the call and *max_chan the largest
 * channel frame not lost.  LC3_ERROR for max_frame_bytes <= 0, the geometry's errors otherwise. */
LC3_Error lc3plus_dec_plan_packed_lenient(int samplerate, int channels, float frame_ms, int hrmode, int n_streams, const int* start, const int* num_bytes,
                                          const int64_t* offsets, int64_t frames_capacity, int max_frame_bytes, const uint8_t* bfi, int n_frames,
                                          uint16_t* eff, uint8_t* lost, uint8_t* invalid, int* end, int* max_chan);
float     lc3plus_dec_batch_last_kernel_ms(lc3plus_dec_batch* batch);
/* the decoder's work buffers, as lc3plus_enc_batch_work_buffer */
LC3_Error lc3plus_dec_batch_work_buffer(lc3plus_dec_batch* batch, int i, const char** name, void** ptr, size_t* bytes, int* elem);
/* checkpoint / resume of the decoders' cross-frame state (overlap-add memory, last good spectrum, LTPF histories, concealment words), as
 * for the encoder batch; the frame sizes are configuration (lc3plus_dec_batch_set_num_bytes), not state */
size_t    lc3plus_dec_batch_state_size(const lc3plus_dec_batch* batch);
LC3_Error lc3plus_dec_batch_get_state(lc3plus_dec_batch* batch, void* state, size_t size);
LC3_Error lc3plus_dec_batch_set_state(lc3plus_dec_batch* batch, const void* state, size_t size);
/* Stream lifecycle of the decoder batch: as for the encoder batch (lc3plus_enc_batch_reset_streams ...).  reset_streams takes num_bytes (NULL keeps each
 * stream's size; otherwise [n] stream-frame sizes, each listed stream configured as set_num_bytes configures it, every size checked first:
 * LC3_NUMBYTES_ERROR).  The reset does not wait for the device, also after decode_sizes_device calls: the listed streams' configuration is written on the
 * device in order, and num_bytes(stream) reads it back as after those calls.  Import does not change configuration (set_num_bytes). */
size_t    lc3plus_dec_batch_stream_state_size(const lc3plus_dec_batch* batch);
LC3_Error lc3plus_dec_batch_reset_streams(lc3plus_dec_batch* batch, const int* streams, int n, const int* num_bytes, void* hip_stream, int sync);
LC3_Error lc3plus_dec_batch_export_streams(lc3plus_dec_batch* batch, const int* streams, int n, void* blob, int blob_on_device, void* hip_stream, int sync);
LC3_Error lc3plus_dec_batch_import_streams(lc3plus_dec_batch* batch, const int* streams, int n, const void* blob, int blob_on_device, uint8_t* status,
                                           void* hip_stream, int sync);
/* The decoder's counterpart of lc3plus_enc_batch_set_input_ready: with ready != 0 the caller guarantees that the frames passed to every
 * following decode() call with device pointers (no bad-frame flags, no status) are COMPLETE in device memory when the call is made.  The
 * bitstream parser of a call - stateless - then runs on a stream of the batch beside the transform and synthesis of the call before; results
 * are identical, and the PCM of a call is complete in stream order on hip_stream as before.  Off by default. */
LC3_Error lc3plus_dec_batch_set_input_ready(lc3plus_dec_batch* batch, int ready);
/* Placed PCM for the decoder's output ("Placed PCM" above): offsets NULL = off. */
LC3_Error lc3plus_dec_batch_set_pcm_placement(lc3plus_dec_batch* batch, const int64_t* offsets, int64_t capacity);
/* Per-stream frame counts for the decoder (jitter: at one tick a stream has three frames waiting, another one, a third none).
 *   counts : device pointer to int32 [n_streams], or NULL = off (the default; every call then behaves as without this function)
 * The setter only records the pointer: it queues nothing and waits for nothing (LC3_NULL_ERROR for a NULL batch).  Counts are configuration, not state:
 * get_state / set_state and the stream blobs do not carry them.  Through lc3plus_dec_sharded_shard() they apply to that shard, with its local stream indices.
 * While counts are set they apply to decode_sizes_device() and decode_packed(); the array is read on the device when the call's kernels run, so a kernel or
 * copy queued earlier on the same hip_stream may produce it (these calls are ordered; no promise is involved).  Every other decode call of the batch -
 * decode(), decode_sizes(), the traced call - returns LC3_ERROR, queues nothing and leaves the batch unchanged; the sharded lc3plus_dec_sharded_decode() and
 * _decode_device() make that check for all shards before any shard is touched.
 *
 * The rule.  With c = min(max(counts[s], 0), n_frames) for a call of n_frames, of stream s
 *   frames t < c are PRESENT: exactly as in the same call without counts - the frame rule with its carry of the last good size and the invalid entries,
 *     concealment, placed PCM with its status bit 2, every PCM format word and layout (LC3PLUS_PCM_CHANNEL_MAJOR: the channel distance stays n_frames);
 *   frames t >= c are ABSENT: their num_bytes, bfi, offsets and placement entries are not looked at, their frame bytes are never read, they are neither
 *     decoded nor concealed, no byte of their PCM is written, and status[s][t] (where status is given) is exactly 8 - bit 3, "absent", and no other bit.
 * After the call the stream's state (overlap memory, LTPF histories, concealment words, last good spectrum) is the state after its c present frames, and its
 * configured size that of its last good present frame, or unchanged where there is none; with c = 0 both are bit for bit what they were.  So a sequence of
 * ragged calls gives each stream the PCM and status that one dense sequence of that stream's present frames gives, and counts that all equal n_frames give
 * the bytes, status and state of the call without counts.  Only a tail can be absent: a count skips no frame in the middle of a call. */
LC3_Error lc3plus_dec_batch_set_frame_counts(lc3plus_dec_batch* batch, const int32_t* counts);
/* The clamp of that rule on the host alone, no device: effective[s] = min(max(counts[s], 0), n_frames).  LC3_NULL_ERROR for a NULL array with n_streams > 0,
 * LC3_ERROR for n_streams < 0 or n_frames <= 0. */
LC3_Error lc3plus_dec_plan_counts(const int32_t* counts, int n_streams, int n_frames, int32_t* effective);

/* ---- Frame probe: what the decoder would do with a frame, and the frame's side information, without decoding ----------------------------------------
 * A receiver that holds two copies of a packet must pick the one that parses before it commits either to a stream - the decoder is stateful and conceals what
 * it refuses; a forwarding server that never decodes wants to drop corrupt packets and to read the per-frame side information (bandwidth, global gain as an
 * activity measure, the LTPF flags, the noise factor).  All of that is in a frame's own bytes.  The probe is a STATELESS call on a decoder batch: it borrows
 * the batch's device, geometry and per-size channel table and nothing else.  It reads and writes no stream state, no configuration and none of the batch's
 * buffers: get_state(), num_bytes(stream) and the PCM and status of every later decode call are bit for bit what they are without it.  It is queued on
 * hip_stream (NULL: the batch's stream), returns at once unless sync, never waits for the device otherwise, and may run on another stream beside a decode call
 * of the same batch.
 *
 *   frames, offsets, num_bytes, info : device pointers.  An ITEM is one stream-frame, all channels; the n_items items are a flat list that has nothing to do with
 *                     the batch's n_streams.  Item i is read from frames + offsets[i] (int64), num_bytes[i] bytes (int32).
 *   info            : [n_items][channels][LC3PLUS_FRAME_INFO_WORDS] int32, one record per channel-frame; no byte behind the n_items records is written
 *   depth           : LC3PLUS_PROBE_SIDE - the side information alone (R/dec_entropy.c:120-270): a few words per channel from the end of its bytes.  Only the
 *                     side information's own checks can refuse (reasons 1 - 4); a frame whose first failure lies in the coded part READS AS ACCEPTED at this
 *                     depth.  tns_order holds the two filter flags (0 / 1), tns_idx and nres are 0.
 *                     LC3PLUS_PROBE_FULL - also the TNS symbols and the whole walk over the spectrum's tuples (R/ari_codec.c:204-509): the verdict is the
 *                     decoder's, the reason any of the eleven, tns_order the decoded orders, nres the residual bits the decoder ends with.
 * The item rule is decode_packed()'s frame rule without flags and without a carry: size 0 is LOST; INVALID is a size outside the geometry's limits for any
 * channel of the split, a size above max_frame_bytes, a negative offset, or offset + size > frames_capacity.  A lost or invalid item is never read; of a good
 * item only the aligned words that hold one of its bytes are read.  A good item's channels are split from its own size as the decoder splits them.
 *
 * The record of a channel-frame (LC3PLUS_FI_*):
 *   [0] status: 0 = the decoder decodes this channel-frame.  Bit 0 (1): it conceals it - set with every other bit, alone where the bitstream is refused; bit 1
 *       (2): the item is invalid; bit 2 (4): the item is lost; bit 3 (8): skipped - a later channel behind a refused earlier one, concealed unparsed
 *       (R/dec_lc3_fl.c:146-160)
 *   [1] the reason LC3PLUS_REJ_* where the status is exactly 1: the first check that fails in the reference's order (for its three returns on the range
 *       decoder's error flag: what set the flag first); 0 otherwise.  lc3plus_reject_name() gives the names.
 *   [2] this channel's byte count (0 for a lost or invalid item)
 *   [3 ...] bw_idx, lastnz, lsb_mode, gg_idx, fac_ns, nfilt, tns_order[2], tns_idx[16], scf_idx[7], ltpf[3], nres - every word 0 where the status is not 0
 *   the rest: 0.
 * Refused calls queue nothing: a NULL batch, frames, offsets, num_bytes or info (LC3_NULL_ERROR); n_items <= 0, max_frame_bytes <= 0, frames_capacity < 0 or a
 * depth other than the two (LC3_ERROR) - checked in that order, before anything of the batch or the device is touched.  The kernels live in
 * liblc3plus_probe_hip.so, which this library loads from its own directory on the first probe call: where that file is missing the call returns LC3_ERROR and
 * nothing else changes.  FULL stages channels of up to 128 bytes in LDS, bounded by ceil(max_frame_bytes / channels): a tight max_frame_bytes keeps that kernel. */
#define LC3PLUS_PROBE_SIDE 0
#define LC3PLUS_PROBE_FULL 1
#define LC3PLUS_FRAME_INFO_WORDS 48
#define LC3PLUS_FI_STATUS     0
#define LC3PLUS_FI_REASON     1
#define LC3PLUS_FI_NUM_BYTES  2
#define LC3PLUS_FI_BW_IDX     3
#define LC3PLUS_FI_LASTNZ     4
#define LC3PLUS_FI_LSB_MODE   5
#define LC3PLUS_FI_GG_IDX     6
#define LC3PLUS_FI_FAC_NS     7
#define LC3PLUS_FI_NFILT      8
#define LC3PLUS_FI_TNS_ORDER  9       /* 2 words */
#define LC3PLUS_FI_TNS_IDX    11      /* 16 words */
#define LC3PLUS_FI_SCF_IDX    27      /* 7 words */
#define LC3PLUS_FI_LTPF       34      /* 3 words: active flag, pitch present, pitch index */
#define LC3PLUS_FI_NRES       37
#define LC3PLUS_FI_ST_CONCEALED 1
#define LC3PLUS_FI_ST_INVALID   2
#define LC3PLUS_FI_ST_LOST      4
#define LC3PLUS_FI_ST_SKIPPED   8
#define LC3PLUS_REJ_NONE          0
#define LC3PLUS_REJ_BANDWIDTH     1   /* bandwidth index above the sampling rate's */
#define LC3PLUS_REJ_LASTNZ        2   /* last non-zero line beyond the coded lines */
#define LC3PLUS_REJ_SNS_INDEX_25  3   /* SNS joint index out of range, 25-bit form */
#define LC3PLUS_REJ_SNS_INDEX_24  4   /* SNS joint index out of range, 24-bit form */
#define LC3PLUS_REJ_TNS_ORDER     5   /* TNS order above the frame length's maximum */
#define LC3PLUS_REJ_TNS_READER    6   /* the backward reader behind the forward one inside the TNS coefficients */
#define LC3PLUS_REJ_TNS_SYMBOL    7   /* range-decoder state invalid on a TNS symbol */
#define LC3PLUS_REJ_OVERLAP       8   /* the two readers overlap by more than 3 bytes inside the spectrum */
#define LC3PLUS_REJ_SPEC_SYMBOL   9   /* range-decoder state invalid inside the spectrum */
#define LC3PLUS_REJ_ESCAPE_14     10  /* escape at level 14 */
#define LC3PLUS_REJ_NRES          11  /* negative residual budget */
#define LC3PLUS_REJ_COUNT         12
LC3_Error lc3plus_dec_batch_probe(lc3plus_dec_batch* batch, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes,
                                  int max_frame_bytes, int64_t n_items, int depth, int32_t* info, void* hip_stream, int sync);
const char* lc3plus_reject_name(int code);      /* "none", "bandwidth", ... for LC3PLUS_REJ_* 0 .. 11, "" otherwise */
/* The SIDE depth on the host alone, no device: the same record rule on one stream-frame in host memory (frame: num_bytes bytes; size 0 is lost, a size the
 * geometry refuses invalid) -> info [channels][LC3PLUS_FRAME_INFO_WORDS].  LC3_NULL_ERROR for a NULL info, or a NULL frame with num_bytes > 0; the geometry's
 * errors otherwise. */
LC3_Error lc3plus_frame_info_side(int samplerate, int channels, float frame_ms, int hrmode, const uint8_t* frame, int num_bytes, int32_t* info);

/* ---- Packet ingest: order, de-duplicate and gap-mark packets on the device -----------------------------------------------------------------------------
 * The probe takes a flat list of items in arrival order - any offsets, any order, duplicates, copies of one packet; decode_packed() takes tables indexed
 * [stream][frame], size 0 for a lost frame, and a count per stream (set_frame_counts).  The ingest call turns the first into the second in device memory, so
 * that probe -> ingest -> set_frame_counts + decode_packed runs on one HIP stream with no host wait in between.
 *
 * Every pointer but `batch` is a device pointer; the inputs are read when the kernels run, so the probe call queued before on the same stream may produce `info`.
 * The call is STATELESS, like the probe: it borrows the batch's device, n_streams and channels and nothing else.  No stream state, configuration or buffer of
 * the batch is read or written, it allocates nothing, and it may run beside a decode call.  It is queued on hip_stream (NULL: the batch's stream) and returns
 * at once unless sync.  No output may overlap an input or another output (next_base must not overlap base).  On a shard's batch
 * (lc3plus_dec_sharded_shard) the call works as on any batch, with that shard's n_streams and LOCAL stream indices; nothing else is needed for sharded batches.
 *
 *   stream, seq, offsets, num_bytes : [n_items] the stream index, sequence number, byte offset (int64, as the probe takes it) and size of each item
 *   info      : the probe's records of the same items [n_items][channels][LC3PLUS_FRAME_INFO_WORDS], or NULL; only each record's status word is read
 *   base      : [n_streams] the sequence number of frame 0 of the coming decode call
 *   floor     : [n_streams] or NULL: frames the stream must advance by at least (a play-out deadline: what has not arrived by now is lost)
 *   seq_bits  : 16 (RTP) or 32: sequence numbers wrap at 2^seq_bits
 *   out_offsets, out_num_bytes, cell_item : [n_streams][n_frames]; the first two are decode_packed()'s offsets and num_bytes.  cell_item is also the call's
 *               workspace
 *   counts    : [n_streams], what set_frame_counts takes
 *   next_base, stats [n_streams][4], item_status [n_items] : each may be NULL
 *
 * Per item i, in this order:
 *   1. stream[i] outside [0, n_streams): BAD_STREAM.
 *   2. num_bytes[i] == 0: EMPTY.  With info, an item also counts as EMPTY if any of its channels' status has LC3PLUS_FI_ST_LOST.
 *   3. The slot distance d = sign_extend((seq[i] - base[s]) mod 2^seq_bits, seq_bits).  d < 0: LATE.  d >= n_frames: EARLY.  Otherwise the item is a candidate
 *      for cell (s, t = d) with a rank: without info 0; with info 0 if every channel's status word is 0 (the decoder decodes it), 2 if any channel has
 *      LC3PLUS_FI_ST_INVALID, 1 otherwise (refused by the bitstream checks).
 * Per cell: the winner is the candidate with the smallest (rank, i) - an accepted copy beats a refused one wherever it sits in the list, among equals the
 *   earliest item wins, and the result is deterministic.  A cell with a winner w gets out_offsets = offsets[w], out_num_bytes = num_bytes[w], cell_item = w: a
 *   refused or invalid sole copy is handed to the decoder as it is, which then does with it exactly what decode_packed() does today.  A cell without a winner
 *   gets out_offsets = 0, out_num_bytes = 0 (lost) and cell_item = -1.
 * Per stream: counts[s] = max(min(max(floor[s], 0), n_frames), 1 + highest t with a winner) - 0 where there is neither a floor nor a winner;
 *   next_base[s] = (base[s] + counts[s]) mod 2^seq_bits; stats[s] = {counts[s], cells t < counts[s] without a winner, LATE items, EARLY items}.
 * item_status[i] carries exactly one of USED, DUPLICATE (a candidate whose cell another item won), LATE, EARLY, BAD_STREAM, EMPTY, and on a USED or DUPLICATE
 *   item also REFUSED (rank 1) or INVALID (rank 2).
 *
 * Refused calls queue nothing, checked in this order before anything of the batch or the device is touched: a NULL batch, stream, seq, offsets, num_bytes,
 * base, out_offsets, out_num_bytes, cell_item or counts (LC3_NULL_ERROR); n_items <= 0, n_items >= 2^29, n_frames <= 0 or a seq_bits other than 16 and 32
 * (LC3_ERROR).  The kernels live in liblc3plus_ingest_hip.so, which this library loads from its own directory on the first ingest call: where that file is
 * missing the call returns LC3_ERROR and nothing else changes. */
#define LC3PLUS_ING_USED        1
#define LC3PLUS_ING_DUPLICATE   2
#define LC3PLUS_ING_LATE        4
#define LC3PLUS_ING_EARLY       8
#define LC3PLUS_ING_BAD_STREAM  16
#define LC3PLUS_ING_EMPTY       32
#define LC3PLUS_ING_REFUSED     64
#define LC3PLUS_ING_INVALID     128
#define LC3PLUS_ING_STATS_WORDS 4
LC3_Error lc3plus_dec_batch_ingest(lc3plus_dec_batch* batch, int64_t n_items, const int32_t* stream, const int32_t* seq, const int64_t* offsets,
                                   const int32_t* num_bytes, const int32_t* info, const int32_t* base, const int32_t* floor, int seq_bits, int n_frames,
                                   int64_t* out_offsets, int32_t* out_num_bytes, int32_t* cell_item, int32_t* counts, int32_t* next_base, int32_t* stats,
                                   uint8_t* item_status, void* hip_stream, int sync);
/* The same rule on the host alone, no device: the same arrays in host memory, n_streams and channels given instead of a batch.  The refusals of the call above
 * in its order, then LC3_ERROR for n_streams <= 0 or channels < 1. */
LC3_Error lc3plus_plan_ingest(int n_streams, int channels, int64_t n_items, const int32_t* stream, const int32_t* seq, const int64_t* offsets,
                              const int32_t* num_bytes, const int32_t* info, const int32_t* base, const int32_t* floor, int seq_bits, int n_frames,
                              int64_t* out_offsets, int32_t* out_num_bytes, int32_t* cell_item, int32_t* counts, int32_t* next_base, int32_t* stats,
                              uint8_t* item_status);

/* ---- Packet egress: frame tables to packet lists and send buffers on the device ------------------------------------------------------------------------
 * The mirror image of the ingest.  encode_packed() leaves tables indexed [stream][frame] in device memory - offsets, num_bytes, flags - and so does the ingest
 * (out_offsets, out_num_bytes, counts); a sender needs a flat list of packets, each with a sequence number, and a forwarding or simulcast server needs every
 * frame once per receiver behind that receiver's header.  The egress call turns the first into the second in device memory, so that
 * set_frame_counts + encode_packed -> egress (a sender) and probe -> ingest -> egress (a forwarder, which never decodes) run on one HIP stream with no host
 * wait in between.  Its list is the item format the probe and the ingest take: egress -> ingest is a closed loop.
 *
 * Every pointer but `batch` is a device pointer; the inputs are read when the kernels run, so the encode_packed or ingest call queued before on the same stream
 * may produce them.  The call is STATELESS, like the probe and the ingest: lc3plus_enc_batch_egress borrows an encoder batch's device and n_streams,
 * lc3plus_dec_batch_egress a decoder batch's, and nothing else.  No stream state, configuration or buffer of the batch is read or written, nothing is
 * allocated - `work` is the only scratch - and the call may run beside an encode or decode call of the same batch.  It is queued on hip_stream (NULL: the
 * batch's stream) and returns at once unless sync.  No output may overlap an input or another output; wire must not overlap frames.  On a shard's batch the
 * call works as on any batch, with that shard's n_streams and LOCAL stream indices.
 *
 *   frames, frames_capacity : the buffer the frames lie in and its size in bytes
 *   offsets, num_bytes : [n_streams][n_frames] each frame's byte offset in frames (int64) and its size; max_frame_bytes: the largest size a frame may have
 *   flags, skip_mask   : [n_streams][n_frames] or NULL; a frame whose flags have a bit of skip_mask is not sent.  A sender passes encode_packed's flags and
 *                        8, its bit for a frame that did not fit out_capacity: that frame's bytes were never written
 *   counts     : [n_streams] or NULL: the frames each stream has in this call (set_frame_counts' array, or the ingest's counts)
 *   route_src  : [n_routes] the source stream of each route, or NULL: route r sends stream r, and n_routes must equal n_streams
 *   seq_base   : [n_routes] the sequence number of frame 0 on each route; seq_bits: 16 (RTP) or 32
 *   order      : LC3PLUS_PACK_STREAM_MAJOR (the list sorted by route, then frame) or LC3PLUS_PACK_FRAME_MAJOR (by frame, then route: time order, for pacing)
 *   wire, wire_capacity, header_room, align : the send buffer, or NULL: in-place mode
 *   pkt_route, pkt_seq, pkt_frame, pkt_offset (int64), pkt_size, pkt_flags (uint8) : the list, n_routes * n_frames entries each
 *   n_packets, wire_total : one int64 each
 *   next_seq [n_routes], stats [n_routes][LC3PLUS_EGR_STATS_WORDS], cell_status [n_routes][n_frames] (uint8)
 *   work       : lc3plus_egress_work_bytes(n_routes, n_frames) bytes, 8-byte aligned; its contents mean nothing before or after the call
 *   pkt_flags, wire_total, next_seq, stats and cell_status may each be NULL.
 *
 * Routes.  A route is one outgoing flow with a sequence space of its own.  Several routes may name one stream (fan-out, simulcast); a stream may have no
 *   route.  A route whose route_src[r] lies outside [0, n_streams) is BAD: it sends nothing, every cell of it has status BAD_ROUTE, next_seq[r] = seq_base[r]
 *   and its stats are 0.
 * Cells.  For s = route_src[r] let c = min(max(counts[s], 0), n_frames), n_frames where counts is NULL.  Cell (r, t) with t >= c is ABSENT: none of its table
 *   entries is looked at.  A cell with t < c is, in this order: LOST where num_bytes[s][t] == 0; INVALID for a negative size, a size above max_frame_bytes, a
 *   negative offset or offset + size > frames_capacity (computed without overflow); SKIPPED where flags is given and flags[s][t] & skip_mask; SENT otherwise.
 *   Only the bytes of SENT cells are ever read.
 * Sequence numbers follow position, not a running count: cell (r, t) has seq = (seq_base[r] + t) mod 2^seq_bits, and next_seq[r] = (seq_base[r] + c) mod
 *   2^seq_bits.  A LOST, INVALID or SKIPPED frame in front of c therefore leaves a hole in the numbers, which the receiver conceals - exactly what the encoder's
 *   stream did, which advanced over the frame, and what makes the egress the inverse of the ingest.
 * The list holds the SENT cells only, compacted, in `order`.  Packet p carries pkt_route, pkt_seq, pkt_frame = t, pkt_offset, pkt_size and pkt_flags;
 *   *n_packets is the list's length, and entries at or behind it are not written.
 * In-place mode, wire == NULL (header_room must be 0 and align 1): pkt_offset = offsets[s][t] and pkt_size the frame's size - the packet is the frame where it
 *   lies; *wire_total is the sum of the sizes; pkt_flags are 0.  No byte is copied.
 * Wire mode: header_room >= 0 (header_room + max_frame_bytes + 4096 must fit an int32) and align a power of two in [1, 4096].  pkt_size = header_room + size;
 *   pkt_offset is the exclusive scan, in list order and from 0, of pkt_size rounded up to align, and *wire_total that scan's end.  A packet fits when
 *   pkt_offset + pkt_size <= wire_capacity: then the frame's bytes are copied to wire + pkt_offset + header_room, and the header_room bytes in front are left to
 *   the caller.  A packet that does not fit stays in the list with pkt_flags = LC3PLUS_EGR_PKT_OVERFLOW (its cell: SENT | OVERFLOW), keeps its number and copies
 *   nothing.  No byte of wire outside [pkt_offset + header_room, pkt_offset + pkt_size) of a fitting packet is modified.  Of frames, only aligned 32-bit words
 *   that hold a byte of a SENT frame are read, as decode_packed() reads them.
 * stats[r] = {c, SENT cells, LOST + INVALID + SKIPPED cells in front of c, SENT cells that overflowed}.  cell_status holds exactly one of SENT, LOST, INVALID,
 *   SKIPPED, ABSENT and BAD_ROUTE, and OVERFLOW beside SENT.
 *
 * Refused calls queue nothing, checked in this order before anything of the batch or the device is touched: a NULL batch, frames, offsets, num_bytes, seq_base,
 * pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, n_packets or work (LC3_NULL_ERROR); then n_frames <= 0, n_routes <= 0, n_routes * n_frames >= 2^31,
 * max_frame_bytes <= 0, frames_capacity < 0, wire_capacity < 0, a bad order, seq_bits, header_room or align, a NULL route_src with n_routes != n_streams, or a
 * work that is not 8-byte aligned (LC3_ERROR).  The kernels live in liblc3plus_egress_hip.so, which this library loads from its own directory on the first
 * egress call: where that file is missing the call returns LC3_ERROR and nothing else changes. */
#define LC3PLUS_EGR_SENT         1
#define LC3PLUS_EGR_LOST         2
#define LC3PLUS_EGR_INVALID      4
#define LC3PLUS_EGR_SKIPPED      8
#define LC3PLUS_EGR_ABSENT       16
#define LC3PLUS_EGR_BAD_ROUTE    32
#define LC3PLUS_EGR_OVERFLOW     64
#define LC3PLUS_EGR_PKT_OVERFLOW 1
#define LC3PLUS_EGR_STATS_WORDS  4
LC3_Error lc3plus_enc_batch_egress(lc3plus_batch* batch,
    int n_frames, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes, int max_frame_bytes,
    const uint8_t* flags, int skip_mask, const int32_t* counts,
    int n_routes, const int32_t* route_src, const int32_t* seq_base, int seq_bits, int order,
    void* wire, int64_t wire_capacity, int header_room, int align,
    int32_t* pkt_route, int32_t* pkt_seq, int32_t* pkt_frame, int64_t* pkt_offset, int32_t* pkt_size, uint8_t* pkt_flags,
    int64_t* n_packets, int64_t* wire_total, int32_t* next_seq, int32_t* stats, uint8_t* cell_status,
    void* work, void* hip_stream, int sync);
LC3_Error lc3plus_dec_batch_egress(lc3plus_dec_batch* batch,
    int n_frames, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes, int max_frame_bytes,
    const uint8_t* flags, int skip_mask, const int32_t* counts,
    int n_routes, const int32_t* route_src, const int32_t* seq_base, int seq_bits, int order,
    void* wire, int64_t wire_capacity, int header_room, int align,
    int32_t* pkt_route, int32_t* pkt_seq, int32_t* pkt_frame, int64_t* pkt_offset, int32_t* pkt_size, uint8_t* pkt_flags,
    int64_t* n_packets, int64_t* wire_total, int32_t* next_seq, int32_t* stats, uint8_t* cell_status,
    void* work, void* hip_stream, int sync);
/* The same rule on the host alone, no device: the same arrays in host memory (work too), n_streams given instead of a batch; in wire mode the frames are
 * copied as the copy kernel copies them.  hip_stream and sync are ignored.  The refusals of the calls above in their order, with n_streams <= 0 (LC3_ERROR)
 * in front of the route_src check. */
LC3_Error lc3plus_plan_egress(int n_streams,
    int n_frames, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes, int max_frame_bytes,
    const uint8_t* flags, int skip_mask, const int32_t* counts,
    int n_routes, const int32_t* route_src, const int32_t* seq_base, int seq_bits, int order,
    void* wire, int64_t wire_capacity, int header_room, int align,
    int32_t* pkt_route, int32_t* pkt_seq, int32_t* pkt_frame, int64_t* pkt_offset, int32_t* pkt_size, uint8_t* pkt_flags,
    int64_t* n_packets, int64_t* wire_total, int32_t* next_seq, int32_t* stats, uint8_t* cell_status,
    void* work, void* hip_stream, int sync);
/* the bytes of `work` for such a call; 0 for arguments the calls refuse */
int64_t lc3plus_egress_work_bytes(int n_routes, int n_frames);

/* ---- RTP framing: parse received datagrams, stamp sent packets, on the device ------------------------------------------------------------------------------
 * The last step to the wire on both sides.  The ingest takes a flat item list of stream index, sequence number, payload offset and payload size; what a NIC
 * path leaves in device memory is datagrams, each an RTP header (RFC 3550 5.1: the fixed header, a CSRC list, a header extension with 5.3.1's length, padding)
 * in front of its payload, from senders known by their SSRC.  The egress leaves header_room bytes in front of every frame of its wire buffer; what goes out
 * is an RTP header there.  lc3plus_dec_batch_rtp_parse turns the first into the second and lc3plus_*_batch_rtp_stamp fills the third, so that
 * datagrams -> parse -> probe -> ingest -> set_frame_counts + decode_packed and encode_packed -> egress -> stamp run on one HIP stream with no host wait.
 * A payload format's own payload header (the LC3plus table of contents is one) stays with the caller: the stamp leaves payload_room untouched bytes between
 * the RTP header and the frame, and the parse skips payload_room bytes.  SRTP is the block "Secure RTP" below; the contents of RTCP packets (SRTCP with them) are
 * not handled.  Several frames per packet are the block "Redundant audio" below: RFC 2198 packets, a primary frame with up to four earlier ones; other
 * aggregations are not handled.
 *
 * Every pointer but `batch` is a device pointer and is read when the kernels run, so the call queued before on the same stream may produce it.  Both calls are
 * STATELESS and allocate nothing: they borrow the batch's device and n_streams and nothing else, no stream state, configuration or buffer of the batch is read
 * or written, and either may run beside an encode or decode call of the same batch.  They are queued on hip_stream (NULL: the batch's stream) and return at
 * once unless sync.  No output may overlap an input or another output.  On a shard's batch they work as on any batch, with that shard's n_streams and LOCAL
 * stream indices.
 *
 * PARSE.  Item i is the datagram ring[dg_offsets[i] .. dg_offsets[i] + dg_sizes[i]); multi-byte fields are big-endian.
 *   ring, ring_capacity   : the buffer the datagrams lie in and its size in bytes
 *   dg_offsets, dg_sizes  : [n_items] each datagram's byte offset in ring (int64) and its size
 *   ssrc_key, ssrc_stream : [n_ssrc] the senders: an SSRC and the stream it feeds, the keys ascending as uint32 (lc3plus_rtp_sort_ssrc brings a table into
 *                           that order)
 *   payload_type          : [n_streams] the payload type each stream accepts, < 0: any; or NULL: any for all
 *   payload_room          : bytes of payload header behind the RTP header that belong to the caller, 0 ... 4096
 *   stream, seq, offsets (int64), num_bytes : [n_items] the item arrays of the ingest and the probe
 *   timestamp [n_items], marker, status (uint8) [n_items], stats [LC3PLUS_RTP_STATS_WORDS] : each may be NULL
 * The first check that fails gives the item's status:
 *   1 RANGE        dg_offsets[i] < 0, dg_sizes[i] < 0 or offset + size > ring_capacity (computed without overflow); such a datagram is never read
 *   2 SHORT        size < 12
 *   3 VERSION      byte 0 >> 6 != 2
 *   4 RTCP         byte 1 in 192 ... 223: an RTCP packet on the same port (RFC 5761 4)
 *   5 HEADER       with h = 12 + 4 * (byte 0 & 15), the CSRC list: h > size; with the X bit (byte 0 & 16) also h + 4 > size, and then, with
 *                  h += 4 + 4 * BE16(at h + 2), the extension: h > size
 *   6 PADDING      with the P bit (byte 0 & 32) pad is the datagram's last byte, else 0: pad == 0 or h + pad > size
 *   7 PAYLOAD_ROOM size - h - pad < payload_room
 *   8 UNKNOWN_SSRC the lower bound of the SSRC (bytes 8 ... 11 as uint32) in ssrc_key is no equal key, or ssrc_stream there lies outside [0, n_streams).  Host
 *                  and device run one search, so a table that is not sorted gives the same answer on both, whatever it is
 *   9 PAYLOAD_TYPE payload_type is given, payload_type[s] >= 0 and it differs from byte 1 & 127
 * An OK item gets stream = s, seq = BE16(bytes 2 .. 3), offsets = dg_offsets[i] + h + payload_room, num_bytes = size - h - pad - payload_room (0 is possible: the
 * ingest calls it EMPTY), timestamp = BE32(bytes 4 .. 7) and marker = byte 1 >> 7.  Every other item gets stream = -1 and 0 everywhere else: the ingest drops it
 * as BAD_STREAM and the probe reads it as lost, so the arrays go to both as they are, with frames = ring and seq_bits = 16.  stats[k] is the number of items
 * with status k; the call zeroes it, and words 10 ... 15 stay 0.  Of a datagram only bytes 0 ... 11, the two bytes of the extension's length and, with the P bit,
 * the last byte are read, and of the ring only aligned 32-bit words that hold such a byte.
 * Refused calls queue nothing, checked in this order before anything of the batch or the device is touched: a NULL batch, ring, dg_offsets, dg_sizes, ssrc_key,
 * ssrc_stream, stream, seq, offsets or num_bytes (LC3_NULL_ERROR); then n_items <= 0, n_items >= 2^29, ring_capacity < 0, n_ssrc <= 0 or a payload_room outside
 * [0, 4096] (LC3_ERROR).
 *
 * STAMP.  For an encoder batch (a sender) or a decoder batch (a forwarder), as the egress has it.  The packet list is the egress's, its wire buffer the egress's
 * wire buffer, header_room the egress's header_room.
 *   max_packets, n_packets : the list arrays' length, and one int64 in device memory: the list's length, read when the kernel runs
 *   pkt_route, pkt_seq, pkt_frame, pkt_offset (int64), pkt_size, pkt_flags (uint8, may be NULL) : the list
 *   ssrc, ts_base, payload_type : [n_routes] each route's SSRC, the timestamp of its frame 0 and its payload type; ts_step: a frame's samples on the RTP clock
 *   marker_mode, cell_status [n_routes][n_frames], resume [n_routes] (uint8), route_stats [n_routes][LC3PLUS_EGR_STATS_WORDS] : see below; the last three may
 *                           be NULL
 *   wire, wire_capacity, header_room, payload_room : header_room >= 12 + payload_room
 *   pkt_status [max_packets] (uint8), next_ts [n_routes], next_resume [n_routes] (uint8) : each may be NULL
 * For each packet p < min(*n_packets, max_packets), with r = pkt_route[p] and t = pkt_frame[p], in this order: ST_BAD_ROUTE where r lies outside [0, n_routes);
 * ST_OVERFLOW where pkt_flags is given and has LC3PLUS_EGR_PKT_OVERFLOW; ST_RANGE where pkt_offset < 0, pkt_size < header_room, pkt_offset + pkt_size >
 * wire_capacity or t lies outside [0, n_frames).  Such a packet writes nothing.  Every other is STAMPED: the 12 bytes at
 * wire + pkt_offset + header_room - payload_room - 12 become 0x80, M << 7 | (payload_type[r] & 127), BE16(pkt_seq & 0xFFFF),
 * BE32(ts_base[r] + t * ts_step mod 2^32), BE32(ssrc[r]).  No other byte of wire is modified: not the payload_room bytes, not the rest of the header room, not the
 * payload.  Entries of pkt_status at or behind *n_packets are not written.
 * M is 0 under LC3PLUS_RTP_MARKER_NEVER.  Under LC3PLUS_RTP_MARKER_AFTER_HOLE, which needs cell_status (the egress's), M is 1 where the packet starts a
 * talkspurt: at t > 0 where cell_status[r][t - 1] lacks LC3PLUS_EGR_SENT, at t == 0 where resume is given and resume[r] != 0.
 * Per route, with c = route_stats[r][0] (the egress's stats) clamped to [0, n_frames], n_frames where route_stats is NULL: next_ts[r] = ts_base[r] + c * ts_step;
 * next_resume[r] = resume[r] (0 for NULL) where c == 0, otherwise 1 where cell (r, c - 1) is not SENT and else 0 - the resume of the next call.
 * Refused calls queue nothing, checked in this order: a NULL batch, n_packets, pkt_route, pkt_seq, pkt_frame, pkt_offset, pkt_size, ssrc, ts_base, payload_type
 * or wire (LC3_NULL_ERROR); then max_packets <= 0, n_routes <= 0, n_frames <= 0, wire_capacity < 0, payload_room < 0, header_room < 12 + payload_room, a bad
 * marker_mode, MARKER_AFTER_HOLE without cell_status, or next_resume without cell_status (LC3_ERROR).
 *
 * The kernels live in liblc3plus_rtp_hip.so, which this library loads from its own directory on the first RTP call: where that file is missing the call
 * returns LC3_ERROR and nothing else changes. */
#define LC3PLUS_RTP_OK            0
#define LC3PLUS_RTP_RANGE         1
#define LC3PLUS_RTP_SHORT         2
#define LC3PLUS_RTP_VERSION       3
#define LC3PLUS_RTP_RTCP          4
#define LC3PLUS_RTP_HEADER        5
#define LC3PLUS_RTP_PADDING       6
#define LC3PLUS_RTP_PAYLOAD_ROOM  7
#define LC3PLUS_RTP_UNKNOWN_SSRC  8
#define LC3PLUS_RTP_PAYLOAD_TYPE  9
#define LC3PLUS_RTP_STATS_WORDS   16
#define LC3PLUS_RTP_STAMPED       1
#define LC3PLUS_RTP_ST_BAD_ROUTE  2
#define LC3PLUS_RTP_ST_OVERFLOW   4
#define LC3PLUS_RTP_ST_RANGE      8
#define LC3PLUS_RTP_MARKER_NEVER      0
#define LC3PLUS_RTP_MARKER_AFTER_HOLE 1
LC3_Error lc3plus_dec_batch_rtp_parse(lc3plus_dec_batch* batch, int64_t n_items,
    const void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes,
    int n_ssrc, const int32_t* ssrc_key, const int32_t* ssrc_stream, const int32_t* payload_type, int payload_room,
    int32_t* stream, int32_t* seq, int64_t* offsets, int32_t* num_bytes, int32_t* timestamp, uint8_t* marker, uint8_t* status, int32_t* stats,
    void* hip_stream, int sync);
/* The same rule on the host alone, no device: the same arrays in host memory, n_streams given instead of a batch; the datagrams are read byte by byte.
 * hip_stream and sync are ignored.  The refusals of the call above in their order, then n_streams <= 0 (LC3_ERROR). */
LC3_Error lc3plus_plan_rtp_parse(int n_streams, int64_t n_items,
    const void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes,
    int n_ssrc, const int32_t* ssrc_key, const int32_t* ssrc_stream, const int32_t* payload_type, int payload_room,
    int32_t* stream, int32_t* seq, int64_t* offsets, int32_t* num_bytes, int32_t* timestamp, uint8_t* marker, uint8_t* status, int32_t* stats,
    void* hip_stream, int sync);
/* Host: sorts an SSRC table of n entries in place, keys ascending as uint32, each key's stream with it.  LC3_NULL_ERROR for a NULL array, LC3_ERROR for
 * n <= 0 and for a key that occurs twice (the table is sorted all the same). */
LC3_Error lc3plus_rtp_sort_ssrc(int n, int32_t* ssrc_key, int32_t* ssrc_stream);
LC3_Error lc3plus_enc_batch_rtp_stamp(lc3plus_batch* batch, int64_t max_packets, const int64_t* n_packets,
    const int32_t* pkt_route, const int32_t* pkt_seq, const int32_t* pkt_frame, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_flags,
    int n_routes, int n_frames, const int32_t* ssrc, const int32_t* ts_base, const int32_t* payload_type, int ts_step,
    int marker_mode, const uint8_t* cell_status, const uint8_t* resume, const int32_t* route_stats,
    void* wire, int64_t wire_capacity, int header_room, int payload_room,
    uint8_t* pkt_status, int32_t* next_ts, uint8_t* next_resume, void* hip_stream, int sync);
LC3_Error lc3plus_dec_batch_rtp_stamp(lc3plus_dec_batch* batch, int64_t max_packets, const int64_t* n_packets,
    const int32_t* pkt_route, const int32_t* pkt_seq, const int32_t* pkt_frame, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_flags,
    int n_routes, int n_frames, const int32_t* ssrc, const int32_t* ts_base, const int32_t* payload_type, int ts_step,
    int marker_mode, const uint8_t* cell_status, const uint8_t* resume, const int32_t* route_stats,
    void* wire, int64_t wire_capacity, int header_room, int payload_room,
    uint8_t* pkt_status, int32_t* next_ts, uint8_t* next_resume, void* hip_stream, int sync);
/* The same rule on the host alone: the same arrays in host memory (n_packets too), no batch.  hip_stream and sync are ignored.  The refusals of the calls above
 * in their order. */
LC3_Error lc3plus_plan_rtp_stamp(int64_t max_packets, const int64_t* n_packets,
    const int32_t* pkt_route, const int32_t* pkt_seq, const int32_t* pkt_frame, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_flags,
    int n_routes, int n_frames, const int32_t* ssrc, const int32_t* ts_base, const int32_t* payload_type, int ts_step,
    int marker_mode, const uint8_t* cell_status, const uint8_t* resume, const int32_t* route_stats,
    void* wire, int64_t wire_capacity, int header_room, int payload_room,
    uint8_t* pkt_status, int32_t* next_ts, uint8_t* next_resume, void* hip_stream, int sync);

/* ---- Redundant audio: pack and unpack RFC 2198 (RED) packets, on the device ---------------------------------------------------------------------------------
 * The answer to a lost packet other than the decoder's concealment: every packet also carries the one to four frames before its own, so a burst of losses up
 * to the depth costs bytes and no audio.  lc3plus_*_batch_red_pack writes such packets behind the in-place egress, lc3plus_dec_batch_red_unpack takes them
 * apart in front of the probe and the ingest, whose one-copy-per-cell rule already lets any copy of a frame fill its cell:
 *   sender    encode_packed -> egress (in place) -> red_pack -> stamp -> protect
 *   forwarder ... -> ingest -> egress (in place) -> red_pack -> stamp
 *   receiver  unprotect -> parse -> red_unpack -> probe -> ingest -> set_frame_counts + decode_packed
 * on one HIP stream with no host wait.  lc3plus_dec_batch_rtcp_stats keeps taking the parse's arrays, not the unpack's: a redundant block is no packet received.
 *
 * Every pointer but `batch` is a device pointer and is read when the kernels run.  The calls are STATELESS and allocate nothing, as the egress and the RTP calls
 * are: they borrow the batch's device and n_streams and nothing else, and may run beside an encode or decode call of the same batch.  They are queued on
 * hip_stream (NULL: the batch's stream) and return at once unless sync.  No output may overlap an input or another output.
 *
 * The payload of a packet with k redundant blocks (RFC 2198 section 3): k headers of four bytes - 1 | PT(7), then a 14-bit timestamp offset and a 10-bit block
 * length, big-endian - one final byte 0 | PT(7), the k blocks oldest first, and the primary frame, which runs to the payload's end.  The RTP header's own
 * payload type is the RED type: the stamp's payload_type[r], as that call stands.
 *
 * PACK.
 *   n_frames, frames, frames_capacity, offsets, num_bytes, max_frame_bytes, flags, skip_mask, counts, n_routes, route_src : the frame tables, as the egress
 *                           call before took them
 *   max_packets, n_packets, pkt_route, pkt_frame : that call's list (in-place mode); its pkt_seq is not needed here, the stamp reads it
 *   max_depth             : 0 ... LC3PLUS_RED_MAX_DEPTH, the most generations a packet carries
 *   depth                 : [n_routes] each route's depth, clamped to [0, max_depth]; or NULL: max_depth for all
 *   block_pt              : [n_routes] the payload type of the blocks and the primary (its low 7 bits)
 *   ts_step               : a frame's samples on the RTP clock, > 0; max_packet_bytes: the size no packet exceeds for the sake of redundancy, >= 0
 *   tail_bytes_in (uint8) [n_streams][max_depth][tail_stride], tail_sizes_in [n_streams][max_depth] : the history the previous call left, both or neither.  Entry g
 *                           is frame g + 1 before frame 0; a size outside 1 ... min(1023, tail_stride) means none.  tail_stride: a multiple of 16, at least
 *                           min(max_frame_bytes, 1023)
 *   tail_bytes_out, tail_sizes_out : the history for the next call, both or neither
 *   wire, wire_capacity, header_room, align : the send buffer, under the constraints of the egress's wire mode (header_room + max_frame_bytes + 4 * 1027 + 1 +
 *                           4096 must fit an int32)
 *   red_offset (int64), red_size, red_flags (uint8), red_blocks (uint8) : [max_packets] the packet records
 *   wire_total : one int64; route_stats : [n_routes][LC3PLUS_RED_STATS_WORDS]
 *   work       : lc3plus_red_work_bytes(max_packets) bytes, 8-byte aligned; its contents mean nothing before or after the call
 *   flags, counts, route_src, depth, the tails, red_flags, red_blocks, wire_total and route_stats may each be NULL.
 * The primary.  For each packet p < min(*n_packets, max_packets), with r = pkt_route[p], t = pkt_frame[p], and s and c the egress's route rule for r: the packet
 *   is BAD where r lies outside [0, n_routes), t outside [0, n_frames), the route is bad, t >= c, or frame (s, t) is not SENT under the egress's cell rule.  A
 *   BAD packet has red_size 0, red_flags LC3PLUS_RED_PKT_BAD and red_blocks 0; it advances nothing, writes nothing and is in no route's stats.
 * The blocks.  Generations j = 1 ... depth are looked at in that order; generation j is frame u = t - j of stream s: at u >= 0 frame (s, u) of the tables, which
 *   exists where its cell is SENT; at u < 0 entry -u - 1 of the stream's tail, which exists where tails are given and its size says so.  A generation that exists
 *   is carried when its size is at most 1023, j * ts_step <= 16383, and header_room + 1 + the primary's size + (4 + size) of every generation carried so far +
 *   4 + its size <= max_packet_bytes; otherwise it is counted as missed, and the generations behind it are still looked at.  The primary is always carried.
 * The record.  red_blocks has bit j - 1 for every carried generation; red_size = header_room + the payload's size; red_offset is the exclusive scan, in list order
 *   and from 0, of red_size rounded up to align, and *wire_total its end.  A packet with red_offset + red_size > wire_capacity keeps its record, gets
 *   LC3PLUS_EGR_PKT_OVERFLOW in red_flags and writes nothing.  Every other packet writes exactly [red_offset + header_room, red_offset + red_size) of wire: the
 *   headers with offset j * ts_step, the block's size and block_pt[r], the final byte, the blocks oldest first, the primary.  Of frames and the tails only
 *   aligned 32-bit words that hold a byte of a copied frame are read.  Entries at or behind *n_packets are not written.
 *   The stamp then takes red_offset, red_size and red_flags as its list's offset, size and flags, with payload_room = 0 (a BAD packet is ST_RANGE there); the
 *   protect calls follow unchanged.
 * route_stats[r] = {packets that are not BAD, blocks carried, bytes of the carried blocks, generations missed}; packets that overflow are counted.
 * Tails.  For stream s with c = min(max(counts[s], 0), n_frames) and g = 0 ... max_depth - 1, u = c - 1 - g: at u >= 0 entry g is frame (s, u) where its cell is
 *   SENT and its size at most 1023, otherwise size 0; at u < 0 it is entry g - c of the tail input, size 0 without one.  The bytes lie at the slot's start.  A
 *   stream with c = 0 hands its history through, so the caller alternates between two tail buffers.
 * Refused calls queue nothing, checked in this order before anything of the batch or the device is touched: a NULL batch, frames, offsets, num_bytes, n_packets,
 * pkt_route, pkt_frame, block_pt, wire, red_offset, red_size or work (LC3_NULL_ERROR); then n_frames <= 0, n_routes <= 0, max_frame_bytes <= 0,
 * frames_capacity < 0, wire_capacity < 0, max_packets <= 0 or >= 2^31, max_depth outside [0, 4], ts_step <= 0, max_packet_bytes < 0, one of a tail's two arrays
 * without the other, a bad tail_stride where max_depth > 0 and a tail is given, a bad header_room or align, a NULL route_src with n_routes != n_streams, or a
 * work that is not 8-byte aligned (LC3_ERROR).
 *
 * UNPACK.  Item i is the payload ring[offsets[i] .. offsets[i] + num_bytes[i]) of stream[i] with sequence number seq[i]: the parse's outputs as they stand.
 *   stream, seq, offsets (int64), num_bytes, timestamp : [n_items]; timestamp may be NULL (taken as 0)
 *   ring, ring_capacity : the buffer the payloads lie in and its size
 *   max_red   : 0 ... 4, the most redundant blocks taken from a packet
 *   block_pt  : [n_streams] the payload type each stream's blocks and primary must have, < 0: any; or NULL: any for all
 *   ts_step   : a frame's samples on the RTP clock, > 0
 *   out_stream, out_seq, out_offsets (int64), out_num_bytes : [n_items * (max_red + 1)] the item arrays of the probe and the ingest
 *   out_timestamp, out_gen (uint8) : of that length, each may be NULL; status (uint8) [n_items] and stats [LC3PLUS_RED_STATS_WORDS] may be NULL
 * Item i owns slots i * (max_red + 1) + k: slot 0 is the primary, slot k >= 1 the k-th redundant header in wire order.  An unused or dropped slot has stream -1
 * and 0 everywhere else: the ingest drops it as BAD_STREAM and the probe reads it as lost, so the arrays go to both as they are.
 * The first check that fails gives the item's status:
 *   1 DROPPED      stream[i] lies outside [0, n_streams): what the parse refused
 *   2 RANGE        offsets[i] < 0, num_bytes[i] < 0 or offset + size > ring_capacity (computed without overflow); such a payload is never read
 *   3 SHORT        the payload ends inside the header list: in front of a header's first byte or inside a header with the F bit; size 0 is SHORT
 *   4 DEPTH        more than max_red headers have the F bit
 *   5 LENGTH       the header bytes plus the block lengths exceed the payload
 *   6 PAYLOAD_TYPE block_pt is given, block_pt[s] >= 0 and it differs from the final byte's type
 * A refused item fills none of its slots.  In an OK item a single block is dropped, in this order, for a type that differs from a block_pt[s] >= 0, for a
 * timestamp offset that is 0 or no multiple of ts_step, and for a length of 0; it is tallied in stats[8], stats[9] or stats[10].  A kept block gets
 * out_seq = (seq - offset / ts_step) mod 2^16, out_timestamp = timestamp - offset, out_gen = offset / ts_step (255 above that), and its place and length in the
 * ring.  The primary gets seq, timestamp, gen 0 and the rest of the payload; a rest of 0 bytes is the ingest's EMPTY.  stats[k], k < 8, is the number of items
 * with status k; the call zeroes stats.  Of a payload only header bytes are read - of a header behind the max_red-th only its first - and of the ring only
 * aligned 32-bit words that hold such a byte; block bytes are never touched.
 * The sequence numbers of blocks assume a sender that numbers by position, as the egress does: a frame's number is the packet's minus its generation.  Placing
 * blocks by timestamp for other senders is not done.
 * Refused calls queue nothing, checked in this order: a NULL batch, stream, seq, offsets, num_bytes, ring, out_stream, out_seq, out_offsets or out_num_bytes
 * (LC3_NULL_ERROR); then n_items <= 0, n_items >= 2^29, ring_capacity < 0, max_red outside [0, 4] or ts_step <= 0 (LC3_ERROR).
 *
 * The kernels live in liblc3plus_red_hip.so, which this library loads from its own directory on the first RED call: where that file is missing the RED calls
 * alone return LC3_ERROR and nothing else changes. */
#define LC3PLUS_RED_MAX_DEPTH      4
#define LC3PLUS_RED_PKT_BAD        2
#define LC3PLUS_RED_STATS_WORDS    4
#define LC3PLUS_RED_OK             0
#define LC3PLUS_RED_DROPPED        1
#define LC3PLUS_RED_RANGE          2
#define LC3PLUS_RED_SHORT          3
#define LC3PLUS_RED_DEPTH          4
#define LC3PLUS_RED_LENGTH         5
#define LC3PLUS_RED_PAYLOAD_TYPE   6
#define LC3PLUS_RED_DROP_TYPE      8
#define LC3PLUS_RED_DROP_OFFSET    9
#define LC3PLUS_RED_DROP_EMPTY     10
#define LC3PLUS_RED_UNPACK_STATS_WORDS 16
LC3_Error lc3plus_enc_batch_red_pack(lc3plus_batch* batch,
    int n_frames, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes, int max_frame_bytes,
    const uint8_t* flags, int skip_mask, const int32_t* counts, int n_routes, const int32_t* route_src,
    int64_t max_packets, const int64_t* n_packets, const int32_t* pkt_route, const int32_t* pkt_frame,
    int max_depth, const int32_t* depth, const int32_t* block_pt, int ts_step, int max_packet_bytes,
    const uint8_t* tail_bytes_in, const int32_t* tail_sizes_in, int tail_stride, uint8_t* tail_bytes_out, int32_t* tail_sizes_out,
    void* wire, int64_t wire_capacity, int header_room, int align,
    int64_t* red_offset, int32_t* red_size, uint8_t* red_flags, uint8_t* red_blocks, int64_t* wire_total, int32_t* route_stats,
    void* work, void* hip_stream, int sync);
LC3_Error lc3plus_dec_batch_red_pack(lc3plus_dec_batch* batch,
    int n_frames, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes, int max_frame_bytes,
    const uint8_t* flags, int skip_mask, const int32_t* counts, int n_routes, const int32_t* route_src,
    int64_t max_packets, const int64_t* n_packets, const int32_t* pkt_route, const int32_t* pkt_frame,
    int max_depth, const int32_t* depth, const int32_t* block_pt, int ts_step, int max_packet_bytes,
    const uint8_t* tail_bytes_in, const int32_t* tail_sizes_in, int tail_stride, uint8_t* tail_bytes_out, int32_t* tail_sizes_out,
    void* wire, int64_t wire_capacity, int header_room, int align,
    int64_t* red_offset, int32_t* red_size, uint8_t* red_flags, uint8_t* red_blocks, int64_t* wire_total, int32_t* route_stats,
    void* work, void* hip_stream, int sync);
/* The same rule on the host alone, no device: the same arrays in host memory (n_packets and work too), n_streams given instead of a batch; the frames are copied
 * as the copy kernel copies them.  hip_stream and sync are ignored.  The refusals of the calls above in their order, with n_streams <= 0 (LC3_ERROR) in front of
 * the route_src check. */
LC3_Error lc3plus_plan_red_pack(int n_streams,
    int n_frames, const void* frames, int64_t frames_capacity, const int64_t* offsets, const int32_t* num_bytes, int max_frame_bytes,
    const uint8_t* flags, int skip_mask, const int32_t* counts, int n_routes, const int32_t* route_src,
    int64_t max_packets, const int64_t* n_packets, const int32_t* pkt_route, const int32_t* pkt_frame,
    int max_depth, const int32_t* depth, const int32_t* block_pt, int ts_step, int max_packet_bytes,
    const uint8_t* tail_bytes_in, const int32_t* tail_sizes_in, int tail_stride, uint8_t* tail_bytes_out, int32_t* tail_sizes_out,
    void* wire, int64_t wire_capacity, int header_room, int align,
    int64_t* red_offset, int32_t* red_size, uint8_t* red_flags, uint8_t* red_blocks, int64_t* wire_total, int32_t* route_stats,
    void* work, void* hip_stream, int sync);
/* the bytes of `work` for such a call; 0 for a max_packets the calls refuse */
int64_t lc3plus_red_work_bytes(int64_t max_packets);
LC3_Error lc3plus_dec_batch_red_unpack(lc3plus_dec_batch* batch, int64_t n_items,
    const int32_t* stream, const int32_t* seq, const int64_t* offsets, const int32_t* num_bytes, const int32_t* timestamp,
    const void* ring, int64_t ring_capacity, int max_red, const int32_t* block_pt, int ts_step,
    int32_t* out_stream, int32_t* out_seq, int64_t* out_offsets, int32_t* out_num_bytes, int32_t* out_timestamp, uint8_t* out_gen, uint8_t* status, int32_t* stats,
    void* hip_stream, int sync);
/* The same rule on the host alone: the same arrays in host memory, n_streams given instead of a batch; the payloads are read byte by byte.  hip_stream and sync
 * are ignored.  The refusals of the call above in their order, then n_streams <= 0 (LC3_ERROR). */
LC3_Error lc3plus_plan_red_unpack(int n_streams, int64_t n_items,
    const int32_t* stream, const int32_t* seq, const int64_t* offsets, const int32_t* num_bytes, const int32_t* timestamp,
    const void* ring, int64_t ring_capacity, int max_red, const int32_t* block_pt, int ts_step,
    int32_t* out_stream, int32_t* out_seq, int64_t* out_offsets, int32_t* out_num_bytes, int32_t* out_timestamp, uint8_t* out_gen, uint8_t* status, int32_t* stats,
    void* hip_stream, int sync);

/* ---- Generic FEC: XOR parity packets out, lost packets back (RFC 5109), on the device ------------------------------------------------------------------------
 * Redundant audio costs one whole extra frame per packet and generation.  One parity packet over k media packets repairs a single loss per group for 1/k of the
 * bytes.  lc3plus_*_batch_fec_encode writes such packets behind the stamp, lc3plus_dec_batch_fec_recover rebuilds lost media packets behind the parse:
 *   sender    ... egress (wire) [-> red_pack] -> stamp -> fec_encode -> stamp (FEC list) -> protect (media), protect (FEC)
 *   receiver  unprotect -> parse (media types) + parse (FEC types) -> fec_recover -> parse (recovered) [-> red_unpack] -> probe -> ingest -> decode_packed
 * all on one HIP stream with no host wait.  NOT HANDLED: interleaved groups on the sender (a group is k consecutive sequence numbers), protection levels above
 * 0, RFC 8627 (FlexFEC), FEC carried inside RED.  Recovery across calls and iterative recovery are lc3plus_dec_batch_fec_repair's (REPAIR below): the recover call
 * knows the items of its own call alone and makes a single pass.
 *
 * THE WIRE FORMAT.  An FEC packet is an RTP packet; its twelve header bytes are the stamp's work.  Its payload is a 10-byte FEC header, one level header and the
 * level-0 payload, all fields big-endian:
 *   byte 0      E(1) L(1) P(1) X(1) CC(4)       byte 1      M(1) PT recovery(7)       bytes 2-3   SN base
 *   bytes 4-7   TS recovery                      bytes 8-9   length recovery
 *   level header: the protection length (16 bits) and the mask, 16 bits with L = 0 and 48 bits with L = 1; its most significant bit is i = 0, and bit i set means
 *   the media packet with sequence number SN base + i mod 2^16 is protected
 * For a protected RTP packet of n bytes its length is n - 12: CSRC list, extension, payload and padding.  The recovery fields are the XOR, over the protected
 * packets, of the low 6 bits of byte 0, of byte 1, of bytes 4 ... 7 and of the 16-bit length.  The protection length plen is the largest of those lengths.  The
 * level-0 payload is the XOR of bytes 12 ... 12 + plen of every protected packet, shorter packets padded with zeros.  E is 0.
 *
 * ENCODE.  Every pointer but `batch` is a device pointer and is read when the kernels run.  The call is STATELESS and allocates nothing; it borrows the batch's
 * device (the encoder form serves a sender, the decoder form a forwarder), is queued on hip_stream (NULL: the batch's stream) and returns at once unless sync.
 *   max_packets, n_packets, pkt_route, pkt_frame, pkt_offset (int64), pkt_size : the list the stamp took
 *   pkt_status         : the stamp's output; NULL: every entry counts as stamped
 *   wire, wire_capacity, header_room, payload_room : as the stamp took them.  The RTP packet of entry p is wire[a .. pkt_offset + pkt_size) with
 *                        a = pkt_offset + header_room - payload_room - 12.  wire is not modified
 *   n_routes, n_frames, seq_base [n_routes] (the egress's), route_stats (the egress's stats, may be NULL): the count c of route r is route_stats[r][0] clamped to
 *                        [0, n_frames], n_frames with route_stats NULL - the stamp's reading
 *   group [n_routes]   : int32, clamped to [0, LC3PLUS_FEC_MAX_GROUP]; 0: no parity for the route.  A kernel of the caller's sets it from the loss fraction of
 *                        the reception reports
 *   flush [n_routes]   : uint8, may be NULL;   fec_seq_base [n_routes] : the sequence number of each route's first FEC packet of this call
 *   state_in, state_out [n_routes][LC3PLUS_FEC_STATE_WORDS] int32 and acc_in, acc_out [n_routes][acc_stride] bytes (acc_stride a multiple of 16): all four or
 *                        none.  They join consecutive calls into one stream: real-time calls are one frame long, so a group spans calls.  The words are FILL
 *                        (positions passed in the open group), K of the open group, SN base, the mask so far, the XOR of header bytes 0-1 (b0 & 63 | b1 << 8),
 *                        the XOR of the timestamps, the XOR of the lengths, the largest length (-1: the group was dropped); the accumulator row is the open
 *                        group's XOR so far, zeros behind the largest length.  An out buffer may not be its in buffer: the caller alternates two.  Without them
 *                        every route starts empty and an open group is dropped at the end.  A state with K outside [1, 16] or FILL outside [1, K) holds no group
 * THE GROUP RULE, pure arithmetic per route.  Position t of route r has sequence number seq_base[r] + t, whether or not a packet exists there.  With F = FILL and
 * K from the state: if F > 0, the first K - F positions complete the carried group; after that groups of k = group[r] positions open one after the other; with
 * k = 0 the remaining positions are unprotected and FILL ends 0.  A group closes when it is full, and after position c - 1 when flush[r] != 0 and its FILL > 0.
 * Position i of a group is mask bit i, L is 0 always, SN base is the sequence number of the group's position 0.  A route with c = 0 hands its state and
 * accumulator through.
 * MEMBERS.  Cell (r, t), t < c, is a member where a list entry p < min(*n_packets, max_packets) names it (the lowest p wins) that is STAMPED (or pkt_status is
 * NULL), lies in wire as the protect call's RANGE has it (pkt_offset >= 0, header_room <= pkt_size <= 2^20, pkt_offset + pkt_size <= wire_capacity) and whose
 * length is at most 65 535.  A hole leaves its mask bit 0.
 * OUTPUT.  One list entry per group that closes in this call, route-major with groups ascending: entry q by an exclusive scan over the routes' closed-group
 * counts; *n_fec (one int64) their number, which may exceed max_fec_packets.  fec_route; fec_seq = fec_seq_base[r] + the index of the group among the route's
 * closed groups of this call; fec_frame the last position of the group in this call (the stamp turns it into the timestamp); fec_offset = q * fec_stride;
 * fec_size = fec_header_room + 14 + plen; fec_flags (uint8, may be NULL); fec_mask (int32, the 16 mask bits as on the wire, may be NULL); next_fec_seq
 * [n_routes] = fec_seq_base[r] + the route's closed groups, which may be the array fec_seq_base itself (in place, as next_seq of the egress), and route_stats_out [n_routes][4] = {groups closed, packets written, media packets protected by them, bytes of level-0 payload}, each may be NULL.
 * An entry with mask 0 is LC3PLUS_FEC_PKT_EMPTY with size 0: it keeps its number and writes nothing, and the stamp refuses it as ST_RANGE.  An entry with
 * fec_size > fec_stride or fec_offset + fec_size > fec_capacity carries LC3PLUS_EGR_PKT_OVERFLOW, keeps its number and writes nothing; an entry with
 * q >= max_fec_packets keeps its number and writes nothing, not even its record.  An open group whose largest length exceeds acc_stride is dropped: its FILL
 * keeps advancing, its mask becomes 0 and it closes as EMPTY (a group closed without a packet written: groups closed less packets written).
 * Every other entry writes exactly fec_wire[fec_offset + fec_header_room, fec_offset + fec_size); fec_header_room >= 12.  No other byte of fec_wire is written;
 * it may not overlap wire.  acc_out and state_out are written whole.  Of wire only aligned 32-bit words that hold a byte of a member packet are read.  The FEC
 * list goes to the stamp as it stands - pkt_seq = fec_seq, pkt_frame = fec_frame, header_room = fec_header_room, payload_room 0, MARKER_NEVER, the caller's FEC
 * SSRC and payload-type arrays - and then to either protect call with contexts of its own.
 *   work : lc3plus_fec_work_bytes(n_routes, n_frames) bytes, 8-byte aligned; it holds the cell-to-entry map; its contents mean nothing before or after the call
 * Refused calls queue nothing, checked in this order: a NULL batch, n_packets, pkt_route, pkt_frame, pkt_offset, pkt_size, wire, seq_base, group, fec_seq_base,
 * fec_wire, n_fec, fec_route, fec_seq, fec_frame, fec_offset, fec_size or work (LC3_NULL_ERROR); then max_packets <= 0 or >= 2^31 - 1, wire_capacity < 0,
 * payload_room < 0, header_room < 12 + payload_room; n_routes <= 0, n_frames <= 0 or n_routes * n_frames >= 2^31; some but not all of state_in, acc_in, state_out
 * and acc_out; with them acc_stride <= 0 or no multiple of 16, a state_out range that intersects state_in's or an acc_out range that intersects acc_in's; fec_capacity < 0, fec_stride <= 0 or > 2^30,
 * fec_header_room < 12 or > 2^20, max_fec_packets <= 0; an fec_wire range that intersects the wire range; a work that is not 8-byte aligned (LC3_ERROR).
 *
 * RECOVER.  For a decoder batch (a receiver).  Every pointer but `batch` is a device pointer.
 *   ring, ring_capacity : the datagrams' bytes; recovered packets are written into it
 *   dg_offsets (int64), dg_sizes [n_items] : the datagrams, with the plain sizes after unprotect
 *   stream, seq [n_items] : the media parse's; stream -1 means not a usable media packet
 *   fec_stream, fec_offsets (int64), fec_num_bytes [n_fec] : the FEC parse's items; the payload there is the FEC header.  These may be the same datagram list
 *                         parsed with the FEC type table
 *   window              : a power of two in [64, 65536];   ssrc [n_streams] : the SSRC written into recovered headers
 *   rec_offset, rec_stride : FEC item f owns ring[rec_offset + f * rec_stride .. + rec_stride); the caller keeps that region of the ring free
 *   rec_dg_offsets (int64), rec_dg_sizes, rec_seq [n_fec]; status (uint8) [n_fec] and stats [LC3PLUS_FEC_STATS_WORDS], each may be NULL
 *   work                : lc3plus_fec_recover_work_bytes(n_streams, window) bytes, 8-byte aligned
 * THE LOOKUP.  A table [n_streams][window] in the workspace holds, at seq & (window - 1), the lowest item index of the stream with that residue.  A wanted packet
 * is present where the table's item has exactly that stream and that sequence number (and its datagram lies in the ring with at least 12 bytes); otherwise it
 * is missing.  So a collision can only turn a recovery into MISSING; it can never forge one.
 * The status of FEC item f is the first check that fails:
 *   1 DROPPED   stream outside [0, n_streams)
 *   2 RANGE     the item lies outside ring (computed without overflow); such an item is never read
 *   3 SHORT     fewer than 14 bytes, or fewer than 18 with the L bit
 *   4 HEADER    E set, mask 0 or protection length 0
 *   5 LENGTH    14 (18) + plen > size
 *   6 COMPLETE  no protected packet is missing
 *   7 MISSING   two or more are missing
 *   8 PARTIAL   the recovered length exceeds plen
 *   9 OVERFLOW  12 + recovered length > rec_stride, or the slot ends behind ring_capacity
 *   0 RECOVERED
 * Bytes behind level 0 (further levels) are ignored.  Both mask widths are handled, so foreign and interleaved senders work.  A RECOVERED item writes its slot:
 * 0x80 | recovered low 6 bits, the recovered byte 1, the missing sequence number, the recovered timestamp, ssrc[s], then the recovered length's bytes of the XOR
 * of the level-0 payload with bytes 12 ... of every present packet, each cut or padded to plen; rec_dg_offsets[f] is the slot, rec_dg_sizes[f] = 12 + length,
 * rec_seq[f] the sequence number.  Every other item gets 0 in all three and writes no byte of the ring: the parse refuses a size-0 datagram as SHORT, so its
 * item is dropped like any other refused one.  stats[k] counts the items of status k; the call zeroes it.  Two FEC items may recover the same packet: the ingest
 * keeps one.
 * Refused calls queue nothing, checked in this order: a NULL batch, ring, dg_offsets, dg_sizes, stream, seq, fec_stream, fec_offsets, fec_num_bytes, ssrc,
 * rec_dg_offsets, rec_dg_sizes, rec_seq or work (LC3_NULL_ERROR); then n_items <= 0 or >= 2^29, ring_capacity < 0, n_fec <= 0 or >= 2^29; a window that is no
 * power of two in [64, 65536]; rec_offset < 0, rec_stride < 12 or > 2^30, a work that is not 8-byte aligned (LC3_ERROR).
 *
 * The kernels live in liblc3plus_fec_hip.so, which this library loads from its own directory on the first FEC call: where that file is missing the FEC calls
 * alone return LC3_ERROR and nothing else changes. */
#define LC3PLUS_FEC_MAX_GROUP      16
#define LC3PLUS_FEC_STATE_WORDS    8
#define LC3PLUS_FEC_PKT_EMPTY      2
#define LC3PLUS_FEC_ROUTE_STATS_WORDS 4
#define LC3PLUS_FEC_RECOVERED      0
#define LC3PLUS_FEC_DROPPED        1
#define LC3PLUS_FEC_RANGE          2
#define LC3PLUS_FEC_SHORT          3
#define LC3PLUS_FEC_HEADER         4
#define LC3PLUS_FEC_LENGTH         5
#define LC3PLUS_FEC_COMPLETE       6
#define LC3PLUS_FEC_MISSING        7
#define LC3PLUS_FEC_PARTIAL        8
#define LC3PLUS_FEC_OVERFLOW       9
#define LC3PLUS_FEC_STATS_WORDS    16
LC3_Error lc3plus_enc_batch_fec_encode(lc3plus_batch* batch,
    int64_t max_packets, const int64_t* n_packets, const int32_t* pkt_route, const int32_t* pkt_frame, const int64_t* pkt_offset, const int32_t* pkt_size,
    const uint8_t* pkt_status, const void* wire, int64_t wire_capacity, int header_room, int payload_room,
    int n_routes, int n_frames, const int32_t* seq_base, const int32_t* route_stats, const int32_t* group, const uint8_t* flush, const int32_t* fec_seq_base,
    const int32_t* state_in, const uint8_t* acc_in, int32_t* state_out, uint8_t* acc_out, int acc_stride,
    void* fec_wire, int64_t fec_capacity, int64_t fec_stride, int fec_header_room,
    int64_t max_fec_packets, int64_t* n_fec, int32_t* fec_route, int32_t* fec_seq, int32_t* fec_frame, int64_t* fec_offset, int32_t* fec_size, uint8_t* fec_flags,
    int32_t* fec_mask, int32_t* next_fec_seq, int32_t* route_stats_out, void* work, void* hip_stream, int sync);
LC3_Error lc3plus_dec_batch_fec_encode(lc3plus_dec_batch* batch,
    int64_t max_packets, const int64_t* n_packets, const int32_t* pkt_route, const int32_t* pkt_frame, const int64_t* pkt_offset, const int32_t* pkt_size,
    const uint8_t* pkt_status, const void* wire, int64_t wire_capacity, int header_room, int payload_room,
    int n_routes, int n_frames, const int32_t* seq_base, const int32_t* route_stats, const int32_t* group, const uint8_t* flush, const int32_t* fec_seq_base,
    const int32_t* state_in, const uint8_t* acc_in, int32_t* state_out, uint8_t* acc_out, int acc_stride,
    void* fec_wire, int64_t fec_capacity, int64_t fec_stride, int fec_header_room,
    int64_t max_fec_packets, int64_t* n_fec, int32_t* fec_route, int32_t* fec_seq, int32_t* fec_frame, int64_t* fec_offset, int32_t* fec_size, uint8_t* fec_flags,
    int32_t* fec_mask, int32_t* next_fec_seq, int32_t* route_stats_out, void* work, void* hip_stream, int sync);
/* The same rule on the host alone, no device: the same arrays in host memory (n_packets, n_fec and work too), no batch; the payloads are XORed byte by byte.
 * hip_stream and sync are ignored.  The refusals of the calls above in their order, less that of the batch. */
LC3_Error lc3plus_plan_fec_encode(
    int64_t max_packets, const int64_t* n_packets, const int32_t* pkt_route, const int32_t* pkt_frame, const int64_t* pkt_offset, const int32_t* pkt_size,
    const uint8_t* pkt_status, const void* wire, int64_t wire_capacity, int header_room, int payload_room,
    int n_routes, int n_frames, const int32_t* seq_base, const int32_t* route_stats, const int32_t* group, const uint8_t* flush, const int32_t* fec_seq_base,
    const int32_t* state_in, const uint8_t* acc_in, int32_t* state_out, uint8_t* acc_out, int acc_stride,
    void* fec_wire, int64_t fec_capacity, int64_t fec_stride, int fec_header_room,
    int64_t max_fec_packets, int64_t* n_fec, int32_t* fec_route, int32_t* fec_seq, int32_t* fec_frame, int64_t* fec_offset, int32_t* fec_size, uint8_t* fec_flags,
    int32_t* fec_mask, int32_t* next_fec_seq, int32_t* route_stats_out, void* work, void* hip_stream, int sync);
/* the bytes of `work` for an encode call and for a recover call; 0 for arguments the calls refuse */
int64_t lc3plus_fec_work_bytes(int n_routes, int n_frames);
int64_t lc3plus_fec_recover_work_bytes(int n_streams, int window);
LC3_Error lc3plus_dec_batch_fec_recover(lc3plus_dec_batch* batch,
    int64_t n_items, void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes, const int32_t* stream, const int32_t* seq,
    int64_t n_fec, const int32_t* fec_stream, const int64_t* fec_offsets, const int32_t* fec_num_bytes, int window, const int32_t* ssrc,
    int64_t rec_offset, int64_t rec_stride, int64_t* rec_dg_offsets, int32_t* rec_dg_sizes, int32_t* rec_seq, uint8_t* status, int32_t* stats, void* work,
    void* hip_stream, int sync);
/* The same rule on the host alone: the same arrays in host memory, n_streams given instead of a batch.  hip_stream and sync are ignored.  The refusals of the
 * call above in their order, then n_streams <= 0 (LC3_ERROR). */
LC3_Error lc3plus_plan_fec_recover(int n_streams,
    int64_t n_items, void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes, const int32_t* stream, const int32_t* seq,
    int64_t n_fec, const int32_t* fec_stream, const int64_t* fec_offsets, const int32_t* fec_num_bytes, int window, const int32_t* ssrc,
    int64_t rec_offset, int64_t rec_stride, int64_t* rec_dg_offsets, int32_t* rec_dg_sizes, int32_t* rec_seq, uint8_t* status, int32_t* stats, void* work,
    void* hip_stream, int sync);

/* REPAIR.  The stateful sibling of RECOVER, for a receiver whose calls are shorter than a group: a real-time receiver makes one-frame calls, so every group of
 * more than one packet closes in a later call than its first members arrived in.  The caller holds, in device memory, a per-stream history of recent media
 * packets and a per-stream store of FEC packets whose groups are not settled yet.  The call admits its arrivals into both, runs up to `passes` recovery passes
 * over the stored FEC packets against the stored media, writes rebuilt packets into the history - where later passes, later calls and the decoder find them - and
 * hands them on as a datagram list for the parse:
 *   receiver  unprotect -> parse + parse -> fec_repair -> parse (rec list) [-> red_unpack] -> probe -> ingest -> decode_packed
 * The library keeps nothing.  Every pointer but `batch` is a device pointer.
 *   n_items, ring, ring_capacity, dg_offsets (int64), dg_sizes, stream, seq : the media parse's arrays, as RECOVER takes them
 *   n_fec, fec_stream, fec_offsets (int64), fec_num_bytes, fec_seq : the FEC parse's items with their own RTP sequence numbers
 *   ssrc [n_streams]    : the SSRC written into rebuilt headers
 *   n_items and n_fec may each be 0 and their arrays then NULL; a call with both 0 only expires and runs passes
 *   med_offset (a multiple of 16), med_slots H (a power of two in [16, 1024]), med_stride (a multiple of 16 in [16, 2^20]) : the media history, inside the ring so
 *                         that a rebuilt packet is parsed, probed, ingested and decoded by offset like any datagram: slot (s, j) is
 *                         ring[med_offset + (s * H + j) * med_stride, + med_stride).  A datagram of a call that holds a byte of that range is RANGE
 *   med_seq, med_size [n_streams][H] int32 : what each slot holds; size 0: nothing
 *   fec_store [n_streams][P][fec_stride] uint8, fec_slots P (a power of two in [4, 256]), fec_stride (a multiple of 16 in [16, 2^20]) : the stored FEC payloads
 *                         from their first header byte;  cell_seq, cell_size [n_streams][P] int32, cell_status [n_streams][P] uint8 : what each cell holds
 *   state [n_streams][LC3PLUS_FEC_REPAIR_STATE_WORDS] int32, read and written in place like med_seq ... cell_status: bit 0 of word 0 the media head is valid,
 *                         bit 1 the FEC head is valid; word 1 the media head, word 2 the FEC head, word 3 zero.  A stream whose valid bit is 0 has no stored
 *                         packet of that kind, whatever the arrays hold: four zero words start a stream afresh and nothing else needs initialising - so a
 *                         caller follows reset_streams
 *   passes              : 1 ... 4
 *   rec_dg_offsets (int64), rec_dg_sizes, rec_seq [n_streams * P], by cell c = s * P + j: nonzero only for a cell that rebuilt a packet in this call, the offset
 *                         its media slot - a datagram list for rtp_parse over the same ring
 *   item_status (uint8) [n_items], fec_status (uint8) [n_fec], stats [LC3PLUS_FEC_STATS_WORDS] : each may be NULL
 *   work                : lc3plus_fec_repair_work_bytes(n_streams, med_slots, fec_slots) bytes, 8-byte aligned; its contents mean nothing before or after
 * THE RULE.  Every step is as if sequential; no outcome depends on scheduling.  Sequence arithmetic is 16-bit serial arithmetic, d(a, b) = (int16)(a - b).  Under
 * a head h a number sn lies BEHIND a window of n slots where d(h, sn) >= n, and AHEAD of the head where d(sn, h) > 0.
 * 1 USABLE.  A media item gets the first of DROPPED (stream outside [0, n_streams)), RANGE (its datagram outside the ring, or with a byte inside the history: the
 *   call would read it while it writes it), SHORT (fewer than 12 bytes), OVERSIZE
 *   (more than med_stride) that applies, and is usable without one.  An FEC item gets the first of RECOVER's checks 1 ... 5 that fails - RANGE also for a byte inside the history -, then OVERSIZE (more than
 *   fec_stride), and is usable without one.
 * 2 HEADS, per stream and kind, over the media space of seq and the FEC space of fec_seq.  With a valid head h: h' = h + max(0, max over the usable items of
 *   d(seq, h)).  Without one: b the number of the lowest-index usable item, h' = b + max(0, max d(seq, b)), and the kind becomes valid.  A kind with no usable
 *   item keeps its state, and one that stays without a head keeps its arrays untouched.
 * 3 EXPIRY.  A stored entry with (h' - seq) & 0xFFFF >= its slot count becomes empty.  A stored FEC cell, whatever its status, is also emptied when every number
 *   its mask names lies behind the media window.  An empty entry has seq 0, size 0 (and status 0).
 * 4 ADMISSION.  A usable item with (h' - seq) & 0xFFFF below the slot count goes to slot seq & (slots - 1); the others are STALE.  Inside the window this map is
 *   one to one, so only copies of one number meet.  Where the slot holds that number already, what is stored stays and the item is DUPLICATE: a packet rebuilt
 *   earlier is not replaced by its late original.  Of several such items in one call the lowest index is stored, the others are DUPLICATE.  A stored media item
 *   copies exactly its size bytes from byte 0 of its RTP header into its slot and no other byte of the slot; a stored FEC item copies exactly its size bytes
 *   and takes cell status MISSING, "not settled yet".
 * 5 PASSES 1 ... passes.  In pass p every cell with status MISSING gets RECOVER's verdict with the members looked up in the media history as it stood when the
 *   pass began.  A member is present where the slot of its number holds exactly that number: a collision can lose a recovery and never forge one.  With no
 *   member missing the cell is COMPLETE.  Otherwise, where a missing number lies behind the media window - the group can never complete - it is EXPIRED.
 *   Otherwise, with two or more missing, or with the one missing number ahead of the media head (or no media head yet), it stays MISSING: a number ahead of the
 *   head may still arrive, and is rebuilt by the first call whose arrivals have moved the head up to it.  Otherwise PARTIAL where the recovered length exceeds the
 *   protection length, OVERFLOW where 12 + length > med_stride, else RECOVERED: the rebuilt packet - the header as RECOVER writes it, with ssrc[s], then the XOR
 *   bytes - goes to the media slot of the missing number, with med_seq, med_size and the cell's rec_* entry.  Where several cells of one pass rebuild the same
 *   number, the lowest cell writes and reports; the others become TWIN and have no rec_* entry.  COMPLETE, RECOVERED, PARTIAL, OVERFLOW, EXPIRED and TWIN are
 *   final: no later pass or call evaluates such a cell again.  All `passes` passes are queued always; a pass behind one that rebuilt nothing changes nothing.
 *   THE DIFFERENCE FROM RECOVER.  On a single call that holds everything, with no window collision and one pass, statuses 0 ... 9 and the rebuilt bytes are
 *   RECOVER's - but for a group whose one missing member is the newest number of its stream: RECOVER rebuilds it (RECOVERED), REPAIR leaves the cell MISSING until
 *   a later call's arrivals move the head up to that number.
 * 6 REPORTS.  item_status: LC3PLUS_FEC_STORED (0) or the reason the media item was not stored.  fec_status: the reason, or the status of the item's cell after the
 *   last pass.  stats[k]: the FEC items of this call with status k, and besides them the cells carried in from earlier calls that settled in this call, counted
 *   under their new status.  stats and the rec_* arrays are zeroed by the call.
 * Refused calls queue nothing, checked in this order: a NULL batch, ring, ssrc, med_seq, med_size, fec_store, cell_seq, cell_size, cell_status, state,
 * rec_dg_offsets, rec_dg_sizes, rec_seq or work; with n_items > 0 dg_offsets, dg_sizes, stream or seq; with n_fec > 0 fec_stream, fec_offsets, fec_num_bytes or
 * fec_seq (LC3_NULL_ERROR); then n_items < 0 or >= 2^29, ring_capacity < 0, n_fec < 0 or >= 2^29; med_offset < 0 or no multiple of 16, med_slots, med_stride;
 * fec_slots, fec_stride; passes; n_streams * H or n_streams * P of 2^31 - 1 or more; a history that ends behind ring_capacity; any overlap among fec_store, the
 * history's range of the ring, med_seq, med_size, cell_seq, cell_size, cell_status and state; a work that is not 8-byte aligned (LC3_ERROR).
 * The kernels live in liblc3plus_repair_hip.so, loaded like the FEC library's on the first repair call. */
/* the repair call's constants, an enumeration (the #define block above is the encode and recover calls', complete as it stands): the words of a stream's state -
 * bit 0 media head valid, bit 1 FEC head valid | media head | FEC head | 0 -, item_status of a stored media item, and the statuses beyond
 * LC3PLUS_FEC_OVERFLOW (9), in the same numbering space and the same stats words */
enum {
    LC3PLUS_FEC_REPAIR_STATE_WORDS = 4,
    LC3PLUS_FEC_STORED = 0,      /* item_status: the media item went into the history */
    LC3PLUS_FEC_STALE = 10,      /* behind the window of its sequence space */
    LC3PLUS_FEC_DUPLICATE = 11,  /* that sequence number is stored already, or a lower item of this call has it */
    LC3PLUS_FEC_OVERSIZE = 12,   /* longer than the slot stride of its store */
    LC3PLUS_FEC_EXPIRED = 13,    /* a missing member lies behind the media window: the group can no longer be repaired */
    LC3PLUS_FEC_TWIN = 14        /* in the same pass a lower cell rebuilt the same packet */
};
/* the bytes of `work` for a repair call; 0 for arguments the call refuses */
int64_t lc3plus_fec_repair_work_bytes(int n_streams, int med_slots, int fec_slots);
LC3_Error lc3plus_dec_batch_fec_repair(lc3plus_dec_batch* batch,
    int64_t n_items, void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes, const int32_t* stream, const int32_t* seq,
    int64_t n_fec, const int32_t* fec_stream, const int64_t* fec_offsets, const int32_t* fec_num_bytes, const int32_t* fec_seq, const int32_t* ssrc,
    int64_t med_offset, int med_slots, int med_stride, int32_t* med_seq, int32_t* med_size,
    void* fec_store, int fec_slots, int fec_stride, int32_t* cell_seq, int32_t* cell_size, uint8_t* cell_status, int32_t* state, int passes,
    int64_t* rec_dg_offsets, int32_t* rec_dg_sizes, int32_t* rec_seq, uint8_t* item_status, uint8_t* fec_status, int32_t* stats, void* work,
    void* hip_stream, int sync);
/* The same rule on the host alone: the same arrays in host memory, n_streams given instead of a batch (n_streams <= 0 is refused with the counts).  hip_stream
 * and sync are ignored. */
LC3_Error lc3plus_plan_fec_repair(int n_streams,
    int64_t n_items, void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes, const int32_t* stream, const int32_t* seq,
    int64_t n_fec, const int32_t* fec_stream, const int64_t* fec_offsets, const int32_t* fec_num_bytes, const int32_t* fec_seq, const int32_t* ssrc,
    int64_t med_offset, int med_slots, int med_stride, int32_t* med_seq, int32_t* med_size,
    void* fec_store, int fec_slots, int fec_stride, int32_t* cell_seq, int32_t* cell_size, uint8_t* cell_status, int32_t* state, int passes,
    int64_t* rec_dg_offsets, int32_t* rec_dg_sizes, int32_t* rec_seq, uint8_t* item_status, uint8_t* fec_status, int32_t* stats, void* work,
    void* hip_stream, int sync);

/* ---- Reception reports: per-stream RTP statistics and RR report blocks, on the device ----------------------------------------------------------------------
 * A receiver owes its senders RTCP reception reports (RFC 3550 6.4): per source the extended highest sequence number, the cumulative loss, the loss fraction
 * of the last interval and the interarrival jitter.  All four follow from what lc3plus_dec_batch_rtp_parse leaves in device memory - stream, seq, timestamp -
 * and the time each datagram arrived.  lc3plus_dec_batch_rtcp_stats takes those arrays as they stand and a state block per stream and gives the advanced state,
 * the 24-byte report blocks in wire order and a status per item, so that datagrams -> parse -> stats runs on one HIP stream with no host wait; the jitter it
 * keeps is also what sizes a jitter buffer, the ingest's floor.  Sender reports, the RR header in front of the blocks, compound packets, SDES and BYE stay with
 * the caller.
 *
 * Every pointer but `batch` is a device pointer and is read when the kernels run.  The call is STATELESS and allocates nothing: it borrows the batch's device
 * and nothing else, no stream state, configuration or buffer of the batch is read or written, and it may run beside a decode call of the same batch.  It is
 * queued on hip_stream (NULL: the batch's stream) and returns at once unless sync.  No output may overlap an input, another output or the workspace, but
 * state_out may BE state_in.
 *   n_items                       : the list's length
 *   stream, seq, timestamp        : [n_items] the parse's arrays.  A stream outside [0, n_streams) (the parse's -1: a refused datagram) is no source's item
 *   arrival                       : [n_items] when datagram i arrived, in the units of its stream's RTP clock, mod 2^32
 *   n_streams, state_in, state_out: [n_streams][LC3PLUS_RR_STATE_WORDS] each source's state before and after.  A zero-filled block is a source that has not
 *                                   started.  n_streams is the call's own: it need not be the batch's
 *   make_report, ssrc, lsr, dlsr  : 0 or 1; with 1, [n_streams] each source's SSRC and the LSR and DLSR words of its block (lsr, dlsr: NULL for 0 everywhere)
 *   blocks                        : [n_streams][LC3PLUS_RR_BLOCK_BYTES] the report blocks, with make_report
 *   ext_seq [n_items], item_status (uint8) [n_items], stream_stats [n_streams][LC3PLUS_RR_STATS_WORDS] : each may be NULL
 *   workspace, workspace_bytes    : scratch of at least lc3plus_rtcp_workspace_bytes(n_items, n_streams) bytes, at any alignment; its contents mean nothing
 *                                   before or after the call
 *
 * THE RULE.  All arithmetic is on uint32 mod 2^32 unless a cast is written.  A state block's words are FLAGS (bit 0, LC3PLUS_RR_STARTED: the source has
 * started; the other bits are kept as they are), BASE_SEQ, MAX_SEQ, CYCLES, BAD_SEQ, RECEIVED, EXPECTED_PRIOR, RECEIVED_PRIOR, TRANSIT, JITTER (LC3PLUS_RR_FLAGS
 * ... LC3PLUS_RR_JITTER = 0 ... 9).  The items of a stream are taken in list order, which is arrival order: the jitter depends on it.  Streams do not touch each
 * other.
 * 1. stream[i] < 0 or >= n_streams: item_status[i] = LC3PLUS_RR_DROPPED (0), ext_seq[i] = 0, and nothing else happens.
 * 2. Otherwise let s = stream[i], q = seq[i] & 0xFFFF, and init_seq(q) be: BASE_SEQ = MAX_SEQ = q, BAD_SEQ = 65537, CYCLES = RECEIVED = RECEIVED_PRIOR =
 *    EXPECTED_PRIOR = 0, bit STARTED set.
 *    - s has not started: init_seq(q).  The item is `first`; its status is LC3PLUS_RR_COUNTED (1).
 *    - Otherwise RFC 3550 A.1 update_seq without probation (a source the caller put into its table is valid from its first packet), with
 *      udelta = (q - MAX_SEQ) & 0xFFFF:
 *        udelta < 3000 (MAX_DROPOUT)        in order: if q < MAX_SEQ then CYCLES += 65536; MAX_SEQ = q.  Status COUNTED.
 *        else udelta <= 65536 - 100         a large jump (100: MAX_MISORDER).  If q == BAD_SEQ: init_seq(q), the item is `first`, status LC3PLUS_RR_RESTART (3).
 *                                           Otherwise BAD_SEQ = (q + 1) & 0xFFFF, status LC3PLUS_RR_JUMP (2), ext_seq[i] = 0, and the item ends here: it is not
 *                                           counted and does not touch the jitter.
 *        else                               a duplicate or a reordered packet: status LC3PLUS_RR_REORDERED (4).
 *    - Every item that did not end as a JUMP is counted: RECEIVED += 1.
 * 3. Jitter (A.8), for counted items: transit = arrival[i] - timestamp[i].  A `first` item - a start or a restart - sets TRANSIT = transit and JITTER = 0.
 *    Every other counted item: d = transit - TRANSIT; TRANSIT = transit; ad = (int32)d < 0 ? 0 - d : d; JITTER += ad - ((JITTER + 8) >> 4).
 * 4. ext_seq[i] of a counted item is CYCLES + q, with the values after step 2, less 65536 where q > MAX_SEQ (a reordered packet from before the wrap).
 * 5. stream_stats[s] is four words, counted from zero in every call: the items counted (LC3PLUS_RR_ST_COUNTED = 0: every status but DROPPED and JUMP), the JUMP
 *    items (1), the RESTART items (2) and the REORDERED items (3) of stream s.  A stream without items gets zeros.
 * 6. With make_report == 1, for every stream after its items (A.3).  A stream that has not started gets 24 zero bytes, and its state stays as it is.
 *    Otherwise
 *        expected = CYCLES + MAX_SEQ - BASE_SEQ + 1
 *        lost     = (int32)(expected - RECEIVED), clamped to [-0x800000, 0x7FFFFF]
 *        ei       = (int32)(expected - EXPECTED_PRIOR);  li = (int32)((expected - EXPECTED_PRIOR) - (RECEIVED - RECEIVED_PRIOR))
 *        fraction = (ei == 0 || li <= 0) ? 0 : min(255, ((int64)li << 8) / ei), the division truncating towards zero as C's; the block holds its low 8 bits
 *        then EXPECTED_PRIOR = expected and RECEIVED_PRIOR = RECEIVED.
 *    RFC 3550's text gives 256 where nothing of an interval arrived, which does not fit the byte: the fraction is capped at 255 here.
 *    The block is 24 bytes, every field big-endian: ssrc[s] (4 bytes); fraction (1); lost as 24 bits, two's complement (3); CYCLES + MAX_SEQ (4);
 *    JITTER >> 4 (4); lsr[s] (4); dlsr[s] (4).  Where blocks is 4-aligned the device writes a block as six aligned words.
 * 7. With make_report == 0 blocks is not written and EXPECTED_PRIOR / RECEIVED_PRIOR stay as they are, so a run split into several calls with the state
 *    carried from each to the next and a report only in the last equals one call over the whole list.
 * Refused calls queue nothing, checked in this order before anything of the batch or the device is touched: a NULL batch, workspace, stream, seq, timestamp,
 * arrival, state_in or state_out, and with make_report != 0 a NULL ssrc or blocks (LC3_NULL_ERROR); then n_items <= 0, n_items >= 2^29, n_streams <= 0, a
 * make_report other than 0 or 1, and workspace_bytes below what lc3plus_rtcp_workspace_bytes answers (LC3_ERROR).
 *
 * The kernels live in liblc3plus_rtcp_hip.so, which this library loads from its own directory on the first call: where that file is missing the call returns
 * LC3_ERROR and nothing else changes. */
#define LC3PLUS_RR_FLAGS           0
#define LC3PLUS_RR_BASE_SEQ        1
#define LC3PLUS_RR_MAX_SEQ         2
#define LC3PLUS_RR_CYCLES          3
#define LC3PLUS_RR_BAD_SEQ         4
#define LC3PLUS_RR_RECEIVED        5
#define LC3PLUS_RR_EXPECTED_PRIOR  6
#define LC3PLUS_RR_RECEIVED_PRIOR  7
#define LC3PLUS_RR_TRANSIT         8
#define LC3PLUS_RR_JITTER          9
#define LC3PLUS_RR_STATE_WORDS     10
#define LC3PLUS_RR_STARTED         1
#define LC3PLUS_RR_DROPPED         0
#define LC3PLUS_RR_COUNTED         1
#define LC3PLUS_RR_JUMP            2
#define LC3PLUS_RR_RESTART         3
#define LC3PLUS_RR_REORDERED       4
#define LC3PLUS_RR_ST_COUNTED      0
#define LC3PLUS_RR_ST_JUMP         1
#define LC3PLUS_RR_ST_RESTART      2
#define LC3PLUS_RR_ST_REORDERED    3
#define LC3PLUS_RR_STATS_WORDS     4
#define LC3PLUS_RR_BLOCK_BYTES     24
#define LC3PLUS_RR_MAX_DROPOUT     3000
#define LC3PLUS_RR_MAX_MISORDER    100
LC3_Error lc3plus_dec_batch_rtcp_stats(lc3plus_dec_batch* batch, int64_t n_items,
    const int32_t* stream, const int32_t* seq, const int32_t* timestamp, const int32_t* arrival,
    int n_streams, const int32_t* state_in, int32_t* state_out,
    int make_report, const int32_t* ssrc, const int32_t* lsr, const int32_t* dlsr, uint8_t* blocks,
    int32_t* ext_seq, uint8_t* item_status, int32_t* stream_stats,
    void* workspace, int64_t workspace_bytes, void* hip_stream, int sync);
/* the bytes of `workspace` for such a call; 0 for an n_items or n_streams the call refuses */
int64_t lc3plus_rtcp_workspace_bytes(int64_t n_items, int n_streams);
/* The same rule on the host alone, no device: the same arrays in host memory, no batch, no workspace, no stream.  The refusals of the call above in their
 * order, less those of the batch and the workspace. */
LC3_Error lc3plus_plan_rtcp_stats(int64_t n_items,
    const int32_t* stream, const int32_t* seq, const int32_t* timestamp, const int32_t* arrival,
    int n_streams, const int32_t* state_in, int32_t* state_out,
    int make_report, const int32_t* ssrc, const int32_t* lsr, const int32_t* dlsr, uint8_t* blocks,
    int32_t* ext_seq, uint8_t* item_status, int32_t* stream_stats);

/* ---- Secure RTP: protect stamped packets, unprotect received datagrams, on the device -------------------------------------------------------------------------
 * RFC 3711 with its default transform, AES_CM_128_HMAC_SHA1_80, and the _32 variant: AES-128 in counter mode over every payload byte, HMAC-SHA1 over every
 * packet, the tag's length (tag_len: 10 or 4 bytes) a parameter.  lc3plus_*_batch_srtp_protect stands behind the stamp and lc3plus_dec_batch_srtp_unprotect in
 * front of the parse, so that encode_packed -> egress -> stamp -> protect and datagrams -> unprotect -> parse -> probe -> ingest run on one HIP stream with no
 * host wait.  The AEAD suites of RFC 7714 are the block "Secure RTP, AEAD" below.  NOT HANDLED: a key derivation rate other than 0, the MKI (master key
 * identifier), SRTCP, header-extension encryption (RFC 6904) and re-keying (a new master key is a new context, made and uploaded by the caller between calls).
 *
 * THE CONTEXT, host only.  lc3plus_srtp_make_context derives the session keys from a master key (16 bytes) and a master salt (14 bytes) by RFC 3711 4.3.1 with
 * key derivation rate 0 - the AES-CM keystream under the master key from the IV (master_salt ^ label << 48) << 16: label 0 the cipher key (16 bytes), label 1
 * the authentication key (20 bytes), label 2 the session salt (14 bytes) - and lays them out as the device reads them, LC3PLUS_SRTP_CTX_WORDS (64) words:
 *   0 .. 43   the 44 round key words of the cipher key (FIPS-197 5.2), each big-endian
 *   44 .. 47  the session salt << 16 as four big-endian words (the fourth ends in 16 zero bits)
 *   48 .. 52  the SHA-1 state behind the block auth_key ^ 36 36 .. (the HMAC's ipad block), 53 .. 57 the state behind auth_key ^ 5C 5C .. (opad): with them a
 *             packet costs its own compressions and one more, not three more
 *   58 .. 63  zero
 * The caller copies contexts to device memory ([n][64] words, one per route or per source).  The library keeps no copy of any key.  LC3_NULL_ERROR for a NULL
 * argument. */
#define LC3PLUS_SRTP_CTX_WORDS     64
LC3_Error lc3plus_srtp_make_context(const uint8_t* master_key, const uint8_t* master_salt, int32_t* ctx);
/* PROTECT.  Every pointer but `batch` is a device pointer and is read when the kernels run.  The call is STATELESS and allocates nothing; it borrows the batch's
 * device and nothing else (the encoder form serves a sender, the decoder form a forwarder, as the stamp has it), is queued on hip_stream (NULL: the batch's
 * stream) and returns at once unless sync.  No output may overlap an input or another output.
 *   max_packets, n_packets (one int64 in device memory), pkt_route, pkt_offset, pkt_size : the egress's packet list as the stamp took it
 *   pkt_status                    : [max_packets] the stamp's output
 *   wire, wire_capacity, header_room, payload_room : as the stamp took them.  wire is not modified
 *   n_routes; ctx [n_routes][64]; roc [n_routes] each route's rollover counter at seq_base[r]; seq_base [n_routes] the egress's; next_seq [n_routes] the
 *                                   egress's output, or NULL
 *   dst, dst_capacity, dst_stride : the destination: packet p goes to dst + p * dst_stride (the egress leaves no room behind a frame, so the call is out of place)
 *   tag_len                       : 10 or 4
 *   out_offset (int64), out_size, out_status (uint8) : [max_packets], written for the packets in front of n_packets
 *   next_roc                      : [n_routes] each route's rollover counter at next_seq[r]; may be NULL, and needs next_seq
 * THE RULE for packet p.  Its RTP packet is wire[a .. pkt_offset + pkt_size) with a = pkt_offset + header_room - payload_room - 12, the address the stamp wrote
 * to, L bytes.  out_offset[p] = p * dst_stride.  The status is the first that applies:
 *   LC3PLUS_SRTP_NOT_STAMPED  pkt_status[p] lacks LC3PLUS_RTP_STAMPED
 *   LC3PLUS_SRTP_BAD_ROUTE    pkt_route[p] outside [0, n_routes)
 *   LC3PLUS_SRTP_RANGE        pkt_offset < 0, pkt_size < header_room, pkt_size > 2^20 or pkt_offset + pkt_size > wire_capacity
 *   LC3PLUS_SRTP_OVERFLOW     L + tag_len > dst_stride, or the slot ends past dst_capacity: (p + 1) * dst_stride > dst_capacity
 *   LC3PLUS_SRTP_PROTECTED    the packet stands at dst + out_offset[p]: the header (12 bytes: the stamp writes CC = 0 and X = 0), the encrypted payload (the
 *                             payload_room bytes and the frame) and the tag; out_size[p] = L + tag_len
 * A packet that is not PROTECTED writes nothing and has out_size 0.  Of dst only the out_size bytes of protected packets are written; the rest of every slot
 * keeps its contents.  SEQ and SSRC are the header's own bytes: what is on the wire is what the IV uses.  With r the route, b = seq_base[r] & 0xFFFF and
 * d = (SEQ - b) & 0xFFFF the packet's rollover counter is ROC_p = roc[r] + ((b + d) >> 16) in 32-bit arithmetic, and
 * next_roc[r] = roc[r] + ((b + ((next_seq[r] - seq_base[r]) & 0xFFFF)) >> 16).  THE CALLER'S CONDITION: a route sends fewer than 65 536 sequence numbers per call.
 * Keystream block j is AES_k(IV + j) with IV = (salt << 16) ^ (SSRC << 64) ^ (index << 16) and index = ROC_p << 16 | SEQ (RFC 3711 4.1.1); the tag is the leftmost
 * tag_len bytes of HMAC-SHA1(k_a, header || ciphertext || ROC_p as 4 big-endian bytes) (4.2).
 * Refused calls queue nothing, checked in this order before anything of the batch or the device is touched: a NULL batch, n_packets, pkt_route, pkt_offset,
 * pkt_size, pkt_status, wire, ctx, roc, seq_base, dst, out_offset, out_size or out_status, a next_roc without next_seq (LC3_NULL_ERROR); then max_packets <= 0
 * or >= 2^29, wire_capacity < 0, payload_room < 0, header_room < 12 + payload_room, n_routes <= 0, dst_capacity < 0, dst_stride <= 0 or > 2^30, a tag_len other
 * than 4 or 10, and a dst range [dst, dst + dst_capacity) that intersects the wire range (LC3_ERROR). */
#define LC3PLUS_SRTP_PROTECTED     1
#define LC3PLUS_SRTP_NOT_STAMPED   2
#define LC3PLUS_SRTP_BAD_ROUTE     4
#define LC3PLUS_SRTP_RANGE         8
#define LC3PLUS_SRTP_OVERFLOW      16
LC3_Error lc3plus_enc_batch_srtp_protect(lc3plus_batch* batch, int64_t max_packets, const int64_t* n_packets,
    const int32_t* pkt_route, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_status,
    const void* wire, int64_t wire_capacity, int header_room, int payload_room,
    int n_routes, const int32_t* ctx, const int32_t* roc, const int32_t* seq_base, const int32_t* next_seq,
    void* dst, int64_t dst_capacity, int64_t dst_stride, int tag_len,
    int64_t* out_offset, int32_t* out_size, uint8_t* out_status, int32_t* next_roc, void* hip_stream, int sync);
LC3_Error lc3plus_dec_batch_srtp_protect(lc3plus_dec_batch* batch, int64_t max_packets, const int64_t* n_packets,
    const int32_t* pkt_route, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_status,
    const void* wire, int64_t wire_capacity, int header_room, int payload_room,
    int n_routes, const int32_t* ctx, const int32_t* roc, const int32_t* seq_base, const int32_t* next_seq,
    void* dst, int64_t dst_capacity, int64_t dst_stride, int tag_len,
    int64_t* out_offset, int32_t* out_size, uint8_t* out_status, int32_t* next_roc, void* hip_stream, int sync);
/* The same rule on the host alone, no device: the same arrays in host memory, no batch, no stream.  The refusals of the calls above in their order, less that
 * of the batch. */
LC3_Error lc3plus_plan_srtp_protect(int64_t max_packets, const int64_t* n_packets,
    const int32_t* pkt_route, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_status,
    const void* wire, int64_t wire_capacity, int header_room, int payload_room,
    int n_routes, const int32_t* ctx, const int32_t* roc, const int32_t* seq_base, const int32_t* next_seq,
    void* dst, int64_t dst_capacity, int64_t dst_stride, int tag_len,
    int64_t* out_offset, int32_t* out_size, uint8_t* out_status, int32_t* next_roc);
/* UNPROTECT runs in front of lc3plus_dec_batch_rtp_parse on the same datagram list: it authenticates every datagram, decrypts the accepted ones IN PLACE in the
 * ring and gives the sizes without the tags, which go to the parse as its dg_sizes.  Device pointers, stateless, allocation-free and queued as above; no
 * output may overlap an input, another output or the workspace, but state_out may BE state_in.  THE CALLER'S CONDITION: the datagrams of one list do not overlap
 * each other in the ring.
 *   n_items, ring, ring_capacity, dg_offsets (int64), dg_sizes : the datagrams, as the parse takes them
 *   n_ssrc, ssrc_key              : [n_ssrc] the sources, ascending as uint32 as for the parse (lc3plus_rtp_sort_ssrc) and searched by its rule
 *   ctx [n_ssrc][64]; state_in, state_out [n_ssrc][LC3PLUS_SRTP_STATE_WORDS] : each source's context and its replay state before and after
 *   tag_len                       : 10 or 4
 *   sizes_out                     : [n_items]
 *   status (uint8) [n_items], index (int64) [n_items], stats [LC3PLUS_SRTP_STATS_WORDS] : each may be NULL
 *   workspace, workspace_bytes    : scratch of at least lc3plus_srtp_workspace_bytes(n_items, n_ssrc) bytes, at any alignment
 * A source's state is 8 words: FLAGS (bit 0, LC3PLUS_SRTP_STARTED; the other bits are kept), ROC, S_L, WIN_LO, WIN_HI and three words kept as they are (zero).
 * top = ROC << 16 | S_L is the highest index accepted so far; bit k of the window WIN_HI << 32 | WIN_LO is set where index top - k was accepted.  A zero-filled
 * block is a source that has not started; the caller may preset its ROC word (a late joiner).
 * THE RULE for item i, the first failing check giving its status (the status is also the index of its word in stats, which counts the items per status):
 * 1. LC3PLUS_SRTP_UN_RANGE, _SHORT (size < 12 + tag_len), _VERSION, _RTCP and _HEADER are the parse's checks with size - tag_len in the size's place.  The P
 *    bit is not looked at: the padding is encrypted.  A size above 2^20 is UN_RANGE as well: keystream block j is AES_k(IV + j) with j in the IV's low 16 bits,
 *    which are zero, so a payload has at most 2^16 blocks (a datagram over UDP has fewer than 2^12).
 * 2. LC3PLUS_SRTP_UNKNOWN_SSRC: the parse's search of ssrc_key.
 * 3. The index estimate of RFC 3711 3.3.1 and Appendix A against the source's state AS IT STOOD WHEN THE CALL BEGAN: v = ROC - 1 where S_L < 32768 and
 *    SEQ - S_L > 32768, v = ROC + 1 where S_L >= 32768 and S_L - 32768 > SEQ, else v = ROC; index = v << 16 | SEQ.  For a source that has not started S_L is
 *    the SEQ of its first item in list order that passed checks 1 and 2, and ROC is the state's ROC word.  A guess of ROC - 1 at ROC == 0 is refused as
 *    LC3PLUS_SRTP_REPLAY_OLD without authentication.
 * 4. For a started source: LC3PLUS_SRTP_REPLAY_OLD where top - index >= 64, LC3PLUS_SRTP_REPLAYED where 0 <= top - index and that bit of the window is set.
 * 5. LC3PLUS_SRTP_AUTH: the datagram's last tag_len bytes do not equal the tag (as in PROTECT) over the bytes in front of them followed by v.  All tag_len bytes
 *    are compared.
 * 6. LC3PLUS_SRTP_OK (0): the payload bytes [h, size - tag_len), h the header's length with CSRCs and extension, are decrypted in place;
 *    sizes_out[i] = size - tag_len; index[i] is the 48-bit index.
 * Every other item has sizes_out[i] = 0, which the parse refuses as SHORT, and index[i] = 0, and not one byte of it is changed.
 * THE STATE AFTER THE CALL.  top' is the largest accepted index of the source where that exceeds top (or the source had not started), else top.  The new window
 * is the old one shifted left by top' - top (zero at 64 or more), ORed with bit top' - index of every accepted item of this call that lies within 64.  Maximum
 * and OR commute, so the result does not depend on the order the items are taken in.  A source with no accepted item keeps its state word for word.
 * THE ONE DEVIATION FROM RFC 3711 3.3.2: the call is stateless inside itself - every item is checked against the state the call began with - so two authentic
 * copies of one packet inside one call are both OK; a copy in a later call is REPLAYED.  This is what lets every item run in a lane of its own, and it costs
 * nothing: the ingest behind the parse keeps one copy per cell.
 * Refused calls queue nothing, checked in this order before anything of the batch or the device is touched: a NULL batch, workspace, ring, dg_offsets,
 * dg_sizes, ssrc_key, ctx, state_in, state_out or sizes_out (LC3_NULL_ERROR); then n_items <= 0 or >= 2^29, ring_capacity < 0, n_ssrc <= 0, a tag_len other
 * than 4 or 10, and workspace_bytes below what lc3plus_srtp_workspace_bytes answers (LC3_ERROR).
 *
 * The kernels live in liblc3plus_srtp_hip.so, which this library loads from its own directory on the first protect or unprotect call: where that file is
 * missing the call returns LC3_ERROR and nothing else changes. */
#define LC3PLUS_SRTP_STATE_WORDS   8
#define LC3PLUS_SRTP_FLAGS         0
#define LC3PLUS_SRTP_ROC           1
#define LC3PLUS_SRTP_S_L           2
#define LC3PLUS_SRTP_WIN_LO        3
#define LC3PLUS_SRTP_WIN_HI        4
#define LC3PLUS_SRTP_STARTED       1
#define LC3PLUS_SRTP_OK            0
#define LC3PLUS_SRTP_UN_RANGE      1
#define LC3PLUS_SRTP_SHORT         2
#define LC3PLUS_SRTP_VERSION       3
#define LC3PLUS_SRTP_RTCP          4
#define LC3PLUS_SRTP_HEADER        5
#define LC3PLUS_SRTP_UNKNOWN_SSRC  6
#define LC3PLUS_SRTP_REPLAY_OLD    7
#define LC3PLUS_SRTP_REPLAYED      8
#define LC3PLUS_SRTP_AUTH          9
#define LC3PLUS_SRTP_STATS_WORDS   16
LC3_Error lc3plus_dec_batch_srtp_unprotect(lc3plus_dec_batch* batch, int64_t n_items,
    void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes,
    int n_ssrc, const int32_t* ssrc_key, const int32_t* ctx, const int32_t* state_in, int32_t* state_out, int tag_len,
    int32_t* sizes_out, uint8_t* status, int64_t* index, int32_t* stats,
    void* workspace, int64_t workspace_bytes, void* hip_stream, int sync);
/* the bytes of `workspace` for such a call; 0 for an n_items or n_ssrc the call refuses */
int64_t lc3plus_srtp_workspace_bytes(int64_t n_items, int n_ssrc);
/* The same rule on the host alone, no device: the same arrays in host memory (the ring is decrypted in place there), no batch, no workspace, no stream.  The
 * refusals of the call above in their order, less those of the batch and the workspace. */
LC3_Error lc3plus_plan_srtp_unprotect(int64_t n_items,
    void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes,
    int n_ssrc, const int32_t* ssrc_key, const int32_t* ctx, const int32_t* state_in, int32_t* state_out, int tag_len,
    int32_t* sizes_out, uint8_t* status, int64_t* index, int32_t* stats);

/* ---- Secure RTP, AEAD: the same calls with AES-GCM ---------------------------------------------------------------------------------------------------------------
 * RFC 7714 with its two suites, AEAD_AES_128_GCM and AEAD_AES_256_GCM: AES in Galois/Counter mode (NIST SP 800-38D) over every payload byte with the header as
 * associated data and a tag of LC3PLUS_SRTP_GCM_TAG_BYTES (16) bytes; the key's size, 16 or 32 bytes, belongs to the context, so routes and sources of both
 * suites stand side by side in one call.  The calls are those of the block "Secure RTP" above without tag_len, and EVERYTHING NOT SAID HERE IS THAT BLOCK'S
 * RULE WORD FOR WORD with the tag length 16: the packet list, wire, header_room and payload_room, dst and dst_stride, roc, seq_base, next_seq and next_roc and
 * the caller's condition on them, LC3PLUS_SRTP_PROTECTED ... _OVERFLOW; the datagram list, the state block of LC3PLUS_SRTP_STATE_WORDS words, the checks 1 to 4
 * and 6 and LC3PLUS_SRTP_OK ... _AUTH (_SHORT is size < 12 + 16), the stats words, the workspace of lc3plus_srtp_workspace_bytes; the state after the call;
 * that the call is stateless inside itself; that a refused datagram keeps every byte; that state_out may be state_in; and the refusals and their order, less
 * that of tag_len.  NOT HANDLED: SRTCP, the MKI, header-extension encryption (RFC 6904), key derivation rates other than 0, re-keying, and the variants with
 * an 8-byte tag that never reached the RFC.
 *
 * THE CONTEXT, host only.  lc3plus_srtp_gcm_make_context derives the session key and salt from a master key (key_bytes: 16 or 32) and a master salt (12 bytes)
 * by RFC 7714 11: the key derivation of RFC 3711 4.3.1 with key derivation rate 0, the master salt followed by two zero bytes in the 14-byte salt's place,
 * the PRF AES-128-CM for a 16-byte master key and AES-256-CM (RFC 6188) for a 32-byte one; label 0 gives the session key (key_bytes bytes), label 2 the session
 * salt (12 bytes), and there is no authentication key.  LC3PLUS_SRTP_GCM_CTX_WORDS (128) words, as the device reads them:
 *   0 .. 59    the round key words of the session key (FIPS-197 5.2), each big-endian: 44 for a 16-byte key (the rest zero), 60 for a 32-byte key
 *   60         the number of rounds, 10 or 14
 *   61 .. 63   the session salt as three big-endian words
 *   64 .. 127  the GHASH table: the sixteen multiples e(x) * H of H = AES_k(0^128), entry e at words 64 + 4 e .. 64 + 4 e + 3, big-endian, a nibble's highest
 *              bit the lowest power (entry 8 is H, entry 4 is H x, entry 2 H x^2, entry 1 H x^3)
 * The caller copies contexts to device memory ([n][128] words, one per route or per source).  The library keeps no copy of any key and wipes its working
 * copies.  LC3_NULL_ERROR for a NULL argument, then LC3_ERROR for a key_bytes other than 16 or 32.
 *
 * THE TRANSFORM (RFC 7714 8.1 and 9).  For a packet with header length h - 12 on the send side, with CSRCs and extension on the receive side - and rollover
 * counter v (ROC_p of PROTECT, the estimate of check 3 of UNPROTECT): the 12-byte IV is (00 00 || SSRC || v || SEQ) XOR the session salt, SSRC and SEQ the
 * header's own bytes; the associated data is the header's h bytes; the plaintext is everything behind it, the payload_room bytes and any padding included.
 * Counter blocks are IV || ctr32: ctr = 1 masks the tag, the payload starts at ctr = 2.  The tag is all 16 bytes of GHASH_H(AAD, C) XOR AES_k(IV || 1); it is
 * appended behind the ciphertext and v is appended nowhere: out_size = L + 16.  ctx is [n_routes][128] or [n_ssrc][128].
 * Check 5 of UNPROTECT compares all 16 bytes behind the ciphertext with the tag over header and ciphertext before one byte of the ring is changed; check 6
 * then decrypts [h, size - 16) in place and sizes_out = size - 16.
 * THE CALLER'S CONDITION: a (key, IV) pair never repeats - no two packets of one key with the same SSRC, v and SEQ - which the caller keeps through roc and
 * seq_base exactly as it keeps the keystream of the block above from repeating.  With GCM a repeat gives away the authentication key as well as the XOR of two
 * plaintexts.
 *
 * The kernels live in liblc3plus_gcm_hip.so, which this library loads from its own directory on the first GCM protect or unprotect call: where that file is
 * missing the call returns LC3_ERROR and nothing else changes. */
/* (the values in parentheses: tests/test_srtp_cpu.py lists the constants of the block above by the pattern "LC3PLUS_SRTP_ name, bare number", and these two are not of it) */
#define LC3PLUS_SRTP_GCM_CTX_WORDS (128)
#define LC3PLUS_SRTP_GCM_TAG_BYTES (16)
LC3_Error lc3plus_srtp_gcm_make_context(const uint8_t* master_key, int key_bytes, const uint8_t* master_salt, int32_t* ctx);
LC3_Error lc3plus_enc_batch_srtp_gcm_protect(lc3plus_batch* batch, int64_t max_packets, const int64_t* n_packets,
    const int32_t* pkt_route, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_status,
    const void* wire, int64_t wire_capacity, int header_room, int payload_room,
    int n_routes, const int32_t* ctx, const int32_t* roc, const int32_t* seq_base, const int32_t* next_seq,
    void* dst, int64_t dst_capacity, int64_t dst_stride,
    int64_t* out_offset, int32_t* out_size, uint8_t* out_status, int32_t* next_roc, void* hip_stream, int sync);
LC3_Error lc3plus_dec_batch_srtp_gcm_protect(lc3plus_dec_batch* batch, int64_t max_packets, const int64_t* n_packets,
    const int32_t* pkt_route, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_status,
    const void* wire, int64_t wire_capacity, int header_room, int payload_room,
    int n_routes, const int32_t* ctx, const int32_t* roc, const int32_t* seq_base, const int32_t* next_seq,
    void* dst, int64_t dst_capacity, int64_t dst_stride,
    int64_t* out_offset, int32_t* out_size, uint8_t* out_status, int32_t* next_roc, void* hip_stream, int sync);
/* the same rule on the host alone, as lc3plus_plan_srtp_protect */
LC3_Error lc3plus_plan_srtp_gcm_protect(int64_t max_packets, const int64_t* n_packets,
    const int32_t* pkt_route, const int64_t* pkt_offset, const int32_t* pkt_size, const uint8_t* pkt_status,
    const void* wire, int64_t wire_capacity, int header_room, int payload_room,
    int n_routes, const int32_t* ctx, const int32_t* roc, const int32_t* seq_base, const int32_t* next_seq,
    void* dst, int64_t dst_capacity, int64_t dst_stride,
    int64_t* out_offset, int32_t* out_size, uint8_t* out_status, int32_t* next_roc);
LC3_Error lc3plus_dec_batch_srtp_gcm_unprotect(lc3plus_dec_batch* batch, int64_t n_items,
    void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes,
    int n_ssrc, const int32_t* ssrc_key, const int32_t* ctx, const int32_t* state_in, int32_t* state_out,
    int32_t* sizes_out, uint8_t* status, int64_t* index, int32_t* stats,
    void* workspace, int64_t workspace_bytes, void* hip_stream, int sync);
/* the same rule on the host alone, as lc3plus_plan_srtp_unprotect */
LC3_Error lc3plus_plan_srtp_gcm_unprotect(int64_t n_items,
    void* ring, int64_t ring_capacity, const int64_t* dg_offsets, const int32_t* dg_sizes,
    int n_ssrc, const int32_t* ssrc_key, const int32_t* ctx, const int32_t* state_in, int32_t* state_out,
    int32_t* sizes_out, uint8_t* status, int64_t* index, int32_t* stats);

/* ---- Sharded batches: one call drives encoders or decoders on several GPUs ------------------------------------------------------------------
 * Streams are independent, so a sharded batch is n_devices ordinary batches, each owning a contiguous block of the n_streams streams on a device of its
 * own; nothing is exchanged between devices.  Stream indices are GLOBAL (0 ... n_streams - 1) and arrays are laid out over all n_streams exactly as the
 * per-batch calls lay them out over theirs; a sharded call gives byte for byte what one unsharded batch of n_streams gives.
 *
 * The split, on the host alone (no device): shard `shard` of `n_shards` owns *count streams from *first.  Contiguous blocks in shard order, sizes differ by
 * at most one, the larger blocks first.  LC3_ERROR for n_streams < 0, n_shards <= 0 or a shard out of range. */
LC3_Error lc3plus_shard_block(int n_streams, int n_shards, int shard, int* first, int* count);

typedef struct lc3plus_sharded     lc3plus_sharded;      /* encoders */
typedef struct lc3plus_dec_sharded lc3plus_dec_sharded;  /* decoders */

/* devices[n_devices]: one shard per entry, in order.  An entry is a HIP device index; the same index may appear more than once (two shards, two contexts,
 * one device).  Everything is checked before a device is touched: NULL devices (LC3_NULL_ERROR); n_devices <= 0, a negative entry or more devices than
 * streams (LC3_ERROR); then the geometry and every rate, with the codes of lc3plus_enc_batch_create.  If a shard cannot be created the ones before it are
 * destroyed; on every error *s is NULL.  One worker thread per shard is started here and joined in destroy; no call starts a thread.
 * A sharded batch is used from one thread at a time, as a batch is; distinct sharded batches (and distinct batches) may be used from different threads at
 * the same time. */
LC3_Error lc3plus_enc_sharded_create(lc3plus_sharded** s, int n_streams, int samplerate, int channels, float frame_ms, int hrmode, const int* bitrates,
                                     const int* devices, int n_devices);
LC3_Error lc3plus_enc_sharded_destroy(lc3plus_sharded* s);
int            lc3plus_enc_sharded_shards(const lc3plus_sharded* s);
/* The shard's batch, borrowed (never destroy it), with LOCAL stream indices (owner()).  Everything a batch can do beyond the calls below - rates and sizes in
 * device memory, packed frames, the stream lifecycle, set_input_ready, last_status, last_records - is reached through it.  A sharded call is complete when
 * it returns (or queued on each shard's stream with sync = 0), so calls on a borrowed batch order with it as they order with that batch's own calls. */
lc3plus_batch* lc3plus_enc_sharded_shard(lc3plus_sharded* s, int shard);
int            lc3plus_enc_sharded_device(const lc3plus_sharded* s, int shard);          /* -1 for a bad argument */
LC3_Error      lc3plus_enc_sharded_owner(const lc3plus_sharded* s, int stream, int* shard, int* local);
int       lc3plus_enc_sharded_input_samples(const lc3plus_sharded* s);
int       lc3plus_enc_sharded_num_bytes(const lc3plus_sharded* s, int stream);
int       lc3plus_enc_sharded_stride(const lc3plus_sharded* s);                          /* max over the shards */
LC3_Error lc3plus_enc_sharded_set_bitrate(lc3plus_sharded* s, int stream, int bitrate);
LC3_Error lc3plus_enc_sharded_set_bandwidth(lc3plus_sharded* s, int stream, int bandwidth);
int       lc3plus_enc_sharded_bandwidth(const lc3plus_sharded* s, int stream);
/* Host pointers.  pcm, bitdepth (the format word, every sample type and layout), n_frames, out and out_stride as lc3plus_enc_batch_encode over n_streams;
 * bandwidths, bitrates, num_bytes: NULL or host [n_streams][n_frames].  Each shard makes the call an unsharded batch would be given for these arguments -
 * encode() without bitrates and bandwidths (num_bytes, if given, is then filled with num_bytes(stream)), encode_bitrates() with bitrates alone,
 * encode_bandwidths() with bandwidths - on its block of every array; the shards' calls run at the same time, one host thread per shard, and the call
 * returns when all are done.  Every check of those calls is made for all shards on the calling thread before any shard is touched: a refused call returns
 * the code the unsharded call gives and changes nothing on any device.  Otherwise the result is LC3_OK if every shard returned it, else the first other code
 * in shard order (LC3_BW_WARNING among them); a failure inside one shard does not stop the others from finishing their call. */
LC3_Error lc3plus_enc_sharded_encode(lc3plus_sharded* s, const void* pcm, int bitdepth, const int* bandwidths, const int* bitrates, int n_frames, void* out,
                                     int out_stride, int* num_bytes);
/* Device pointers: pcm[n_shards] and out[n_shards], each on its shard's device and holding that shard's block (pcm[k]: [count_k][n_frames]..., out[k]:
 * [count_k][n_frames][out_stride]); hip_streams: NULL, or [n_shards] streams (an entry may be NULL: the shard's own stream).  Checked for all shards first,
 * as above; then every shard's call is queued before any is waited for.  sync = 0 returns after queueing, sync != 0 when every shard has finished. */
LC3_Error lc3plus_enc_sharded_encode_device(lc3plus_sharded* s, const void* const* pcm, int bitdepth, int n_frames, void* const* out, int out_stride,
                                            void* const* hip_streams, int sync);
/* Checkpoint / resume: the shards' states one after the other in shard order.  A batch's state is [channel-stream][state words], so this IS the state of an
 * unsharded batch of n_streams (state_size() is equal): a checkpoint moves between a sharded batch, an unsharded batch and a sharded batch with another
 * number of shards.  size must be state_size() (LC3_ERROR, nothing written). */
size_t    lc3plus_enc_sharded_state_size(const lc3plus_sharded* s);
LC3_Error lc3plus_enc_sharded_get_state(lc3plus_sharded* s, void* state, size_t size);
LC3_Error lc3plus_enc_sharded_set_state(lc3plus_sharded* s, const void* state, size_t size);
float     lc3plus_enc_sharded_last_kernel_ms(lc3plus_sharded* s, int shard);

/* The decoder twin, with the codes of lc3plus_dec_batch_create (num_bytes may be NULL). */
LC3_Error lc3plus_dec_sharded_create(lc3plus_dec_sharded** s, int n_streams, int samplerate, int channels, float frame_ms, int hrmode, const int* num_bytes,
                                     const int* devices, int n_devices);
LC3_Error lc3plus_dec_sharded_destroy(lc3plus_dec_sharded* s);
int                lc3plus_dec_sharded_shards(const lc3plus_dec_sharded* s);
lc3plus_dec_batch* lc3plus_dec_sharded_shard(lc3plus_dec_sharded* s, int shard);         /* borrowed; local stream indices */
int                lc3plus_dec_sharded_device(const lc3plus_dec_sharded* s, int shard);
LC3_Error          lc3plus_dec_sharded_owner(const lc3plus_dec_sharded* s, int stream, int* shard, int* local);
int       lc3plus_dec_sharded_output_samples(const lc3plus_dec_sharded* s);
int       lc3plus_dec_sharded_delay(const lc3plus_dec_sharded* s);
int       lc3plus_dec_sharded_num_bytes(const lc3plus_dec_sharded* s, int stream);
LC3_Error lc3plus_dec_sharded_set_num_bytes(lc3plus_dec_sharded* s, int stream, int num_bytes);
/* Host pointers, over n_streams: num_bytes NULL -> each shard calls lc3plus_dec_batch_decode, else lc3plus_dec_batch_decode_sizes; bfi and status NULL or
 * [n_streams][n_frames].  Checks, threads and result as lc3plus_enc_sharded_encode. */
LC3_Error lc3plus_dec_sharded_decode(lc3plus_dec_sharded* s, const void* frames, int in_stride, const int* num_bytes, const uint8_t* bfi, int n_frames, void* pcm,
                                     int bps, uint8_t* status);
/* Device pointers, one per shard (frames[k]: [count_k][n_frames][in_stride], pcm[k]: that shard's block), as lc3plus_enc_sharded_encode_device. */
LC3_Error lc3plus_dec_sharded_decode_device(lc3plus_dec_sharded* s, const void* const* frames, int in_stride, int n_frames, void* const* pcm, int bps,
                                            void* const* hip_streams, int sync);
size_t    lc3plus_dec_sharded_state_size(const lc3plus_dec_sharded* s);
LC3_Error lc3plus_dec_sharded_get_state(lc3plus_dec_sharded* s, void* state, size_t size);
LC3_Error lc3plus_dec_sharded_set_state(lc3plus_dec_sharded* s, const void* state, size_t size);
float     lc3plus_dec_sharded_last_kernel_ms(lc3plus_dec_sharded* s, int shard);

/* lc3plus_enc_* spellings of the single-stream API (north-star wording); thin aliases. */
LC3_Error lc3plus_enc_init(LC3_Enc* e, int samplerate, int channels);
LC3_Error lc3plus_enc_set_frame_ms(LC3_Enc* e, float frame_ms);
LC3_Error lc3plus_enc_set_hrmode(LC3_Enc* e, int hrmode);
LC3_Error lc3plus_enc_set_bitrate(LC3_Enc* e, int bitrate);
LC3_Error lc3plus_enc16(LC3_Enc* e, int16_t** input_samples, void* output_bytes, int* num_bytes);
int       lc3plus_enc_get_size(int samplerate, int channels);

#ifdef __cplusplus
}
#endif
#endif
