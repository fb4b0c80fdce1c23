/* lc3_probe_shim.h -- the frame probe (include/lc3plus_batch.h: lc3plus_dec_batch_probe, lc3plus_frame_info_side): what the host C code (lc3_packet.c; lc3_host.c for lc3plus_frame_info_side) and the
 * sibling library that holds the probe kernels (lc3_probe.hip -> liblc3plus_probe_hip.so) share.  The record layout, the item rule and the side-information parse
 * are one text for the host function and the kernels; the lc3probe_* functions are the sibling's whole C ABI.  lc3_packet.c loads the sibling from its own
 * directory on the first probe call; the codec library's own code object holds none of this. */
#ifndef LC3_PROBE_SHIM_H
#define LC3_PROBE_SHIM_H
#include <stdint.h>
#include <stddef.h>
#include "lc3_plan.h"

/* the record of one channel-frame: LC3PLUS_FI_* of include/lc3plus_batch.h */
#define LC3P_WORDS 48
enum { LC3P_STATUS = 0, LC3P_REASON = 1, LC3P_NBYTES = 2, LC3P_BW = 3, LC3P_LASTNZ = 4, LC3P_LSB = 5, LC3P_GG = 6, LC3P_FAC_NS = 7, LC3P_NFILT = 8,
       LC3P_TNS_ORDER = 9, LC3P_TNS_IDX = 11, LC3P_SCF = 27, LC3P_LTPF = 34, LC3P_NRES = 37, LC3P_USED = 38 };
enum { LC3P_ST_CONCEALED = 1, LC3P_ST_INVALID = 2, LC3P_ST_LOST = 4, LC3P_ST_SKIPPED = 8 };
/* LC3PLUS_REJ_*: numbered as the reference's decisions are in oracle/lc3_oracle.h (R/dec_entropy.c:120-270, R/ari_codec.c:204-509) */
enum { LC3P_REJ_NONE = 0, LC3P_REJ_BANDWIDTH, LC3P_REJ_LASTNZ, LC3P_REJ_SNS_INDEX_25, LC3P_REJ_SNS_INDEX_24, LC3P_REJ_TNS_ORDER, LC3P_REJ_TNS_READER,
       LC3P_REJ_TNS_SYMBOL, LC3P_REJ_OVERLAP, LC3P_REJ_SPEC_SYMBOL, LC3P_REJ_ESCAPE_14, LC3P_REJ_NRES, LC3P_REJ_COUNT };
enum { LC3P_DEPTH_SIDE = 0, LC3P_DEPTH_FULL = 1 };
#define LC3P_TAIL_BYTES 12               /* dec_side reads at most 3 + 9 + 1 + 8 + 2 + 1 + 10 + 1 + 2 + 1 + 25 + 10 + 3 = 76 bits from the end of a channel's bytes; no frame is shorter than 20 */

/* The item rule: lc3d_dec_frame_class_packed without a flag and without a carry.  -> LC3D_FRAME_GOOD, _LOST (size 0) or _BAD_SIZE (invalid). */
static inline LC3D_HD int lc3p_item_class(int nb, long long off, long long cap, int max_bytes, const lc3d_dchan* tab, int tab_n, int channels)
{
    return lc3d_dec_frame_class_packed(nb, 0, off, cap, max_bytes, tab, tab_n, channels);
}
/* bytes of channel ch of a good item of fsz bytes, and where they start inside it (R/dec_lc3_fl.c:148) */
static inline LC3D_HD int lc3p_chan_bytes(int fsz, int channels, int ch) { return (fsz + channels - 1 - ch) >> (channels - 1); }
static inline LC3D_HD int lc3p_chan_off(int fsz, int ch) { return ch ? (fsz + 1) >> 1 : 0; }

/* n <= 25 bits from backward bit q on.  v: the last LC3P_TAIL_BYTES bytes of the channel as a 96-bit number, backward bit q (bit (q & 7) of byte
 * nbytes - 1 - (q >> 3)) at bit q: v[0] = byte[nbytes - 1] | byte[nbytes - 2] << 8 | ... */
static inline LC3D_HD int lc3p_bits(uint32_t v0, uint32_t v1, uint32_t v2, int q, int n)
{
    const int i = q >> 5, s = q & 31;
    const uint32_t lo = i == 0 ? v0 : i == 1 ? v1 : v2, hi = i == 0 ? v1 : i == 1 ? v2 : 0u;
    const uint64_t w = ((uint64_t)hi << 32) | lo;
    return (int)((uint32_t)(w >> s) & ((1u << n) - 1u));
}
/* Side information R/dec_entropy.c:120-270 of one channel, the checks in the reference's order: the first that fails is the reason returned and nothing
 * behind it is read.  Accepted (0): rec[LC3P_BW ... LC3P_LTPF + 2] hold the fields with the meaning of lc3d_dec_trace (tns_order: the two flags), *Q the bits read.
 * Refused: rec is as it came. */
static inline LC3D_HD int lc3p_side(uint32_t v0, uint32_t v1, uint32_t v2, int fs_idx, int bw_bits, int ylen, int dms, int32_t* rec, int* Q)
{
    int q = 0, bw = fs_idx;
    if (bw_bits > 0) { bw = lc3p_bits(v0, v1, v2, q, bw_bits); q += bw_bits; if (fs_idx < bw) return LC3P_REJ_BANDWIDTH; }
    const int nfilt = (bw < 3 || dms == 25) ? 1 : 2;
    int nb = 0;
    while ((1 << nb) < ylen / 2) nb++;                                  /* ceil(log2(ylen / 2)) */
    const int lastnz = (lc3p_bits(v0, v1, v2, q, nb) + 1) * 2; q += nb;
    if (lastnz > ylen) return LC3P_REJ_LASTNZ;
    const int lsb = lc3p_bits(v0, v1, v2, q, 1); q += 1;
    const int gg = lc3p_bits(v0, v1, v2, q, 8); q += 8;
    const int ord0 = lc3p_bits(v0, v1, v2, q, 1); q += 1;
    int ord1 = 0;
    if (nfilt == 2) { ord1 = lc3p_bits(v0, v1, v2, q, 1); q += 1; }
    const int lt0 = lc3p_bits(v0, v1, v2, q, 1); q += 1;
    const int s0 = lc3p_bits(v0, v1, v2, q, 5), s1 = lc3p_bits(v0, v1, v2, q + 5, 5); q += 10;
    const int msb = lc3p_bits(v0, v1, v2, q, 1); q += 1;
    int s2 = msb * 2;
    int s3 = lc3p_bits(v0, v1, v2, q, 1 + msb); q += 1 + msb;
    const int s4 = lc3p_bits(v0, v1, v2, q, 1); q += 1;
    int s5 = 0, s6 = 0, lsbm = 0;
    if (msb == 0) {
        const int tt = lc3p_bits(v0, v1, v2, q, 25); q += 25;
        if (tt >= 33460056) return LC3P_REJ_SNS_INDEX_25;
        const int ind = tt / 2390004;
        s5 = tt - ind * 2390004;
        if (ind < 2) { lsbm = 1; s3 = s3 * 2 + ind; s6 = -2; } else { lsbm = 0; s6 = ind - 2; }
    } else {
        const int tt = lc3p_bits(v0, v1, v2, q, 24); q += 24;
        if (tt >= 16708096) return LC3P_REJ_SNS_INDEX_24;
        if (tt >= 15158272) { lsbm = 1; s3 = s3 * 2 + ((tt - 15158272) & 1); s5 = (tt - 15158272) / 2; s6 = -2; } else { lsbm = 0; s5 = tt; s6 = -1; }
    }
    s2 += lsbm;
    int lt1 = 0, lt2 = 0;
    if (lt0 == 1) { lt1 = lc3p_bits(v0, v1, v2, q, 1); lt2 = lc3p_bits(v0, v1, v2, q + 1, 9); q += 10; }
    const int fac = lc3p_bits(v0, v1, v2, q, 3); q += 3;
    rec[LC3P_BW] = bw; rec[LC3P_LASTNZ] = lastnz; rec[LC3P_LSB] = lsb; rec[LC3P_GG] = gg; rec[LC3P_FAC_NS] = fac; rec[LC3P_NFILT] = nfilt;
    rec[LC3P_TNS_ORDER] = ord0; rec[LC3P_TNS_ORDER + 1] = ord1;
    rec[LC3P_SCF] = s0; rec[LC3P_SCF + 1] = s1; rec[LC3P_SCF + 2] = s2; rec[LC3P_SCF + 3] = s3; rec[LC3P_SCF + 4] = s4; rec[LC3P_SCF + 5] = s5; rec[LC3P_SCF + 6] = s6;
    rec[LC3P_LTPF] = lt0; rec[LC3P_LTPF + 1] = lt1; rec[LC3P_LTPF + 2] = lt2;
    *Q = q;
    return LC3P_REJ_NONE;
}

/* what the probe borrows of a decoder batch (lc3_shim.h: lc3hip_dec_probe_args) plus the item list: every pointer but the struct itself is a device pointer */
typedef struct {
    int32_t device, channels, ylen, tab_n;
    const lc3d_plan* plan; const lc3d_dchan* tab;
    const void* frames; long long capacity; const long long* offsets; const int32_t* num_bytes; int32_t max_bytes, depth; long long n_items;
    int32_t* info; void* stream; int32_t sync;
} lc3probe_call;

#ifdef __cplusplus
extern "C" {
#endif
/* queues the probe kernel of q->depth on q->stream; waits for it only with q->sync.  0, or 1 where nothing was queued */
int lc3probe_run(const lc3probe_call* q);
/* launches of a probe kernel by this process, by the kernel's symbol name in the code object; -1 for a name the library does not hold */
long long lc3probe_launch_count(const char* kernel);
#ifdef __cplusplus
}
#endif
#endif
