/* lc3_enc_pack.inc -- second encoder kernel: the bitstream writer, one channel-frame per LANE (included by lc3_kernels.hip).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  Side information (R/enc_entropy.c:13-115), TNS symbols, spectral tuples
 * with escapes / signs / LSB-mode bits, residual bits and the range coder with its cache / carry state machine and finalisation
 * (R/ari_codec.c:511-800) are serial inside a frame, but a frame's bitstream depends on nothing but that frame's quantised spectrum
 * and parameters: lc3_encode_kernel leaves both in a record per channel-frame (PK_* in lc3_plan.h) and this kernel writes the
 * bytes of all B x T frames of the launch at once - 64 frames per wave share one instruction stream instead of one wave walking a
 * frame's ~250 symbols with a single lane's worth of work.  The coder here is the reference's own serial algorithm, per lane.
 *
 * Data: nothing of the frame is staged.  The two write cursors of a frame - range-coder bytes growing forward from byte 0,
 * side / sign / LSB / residual bits growing backward from the last byte (R/enc_entropy.c:101-115) - each keep ONE 32-bit word in a
 * register and store it to the output buffer when it is complete: forward words at frame offset 4k, backward words as the
 * byte-swapped words of the reversed frame (bit q of the backward string = little-endian bit q of the reversed frame), at frame
 * offset nbytes - 4 - 4m, which need not be 4-aligned (gfx950 stores unaligned dwords).  A complete word belongs to one cursor
 * only (the bit budget keeps the cursors apart, R/quantize_spec.c:155-158, R/ari_codec.c:764-780); the two partial words, the byte
 * both cursors may share after finalisation (R/ari_codec.c:573-630) and the unused bytes between them are written bytewise at the
 * end.  So the writer needs no LDS per frame and handles every frame size (20 ... 625 bytes) at four waves per SIMD; the LSB-mode
 * list is appended to the (otherwise unused) residual words of the record; context table and models are gathered from LDS, shared
 * by the four waves of a workgroup. */

struct __attribute__((aligned(16))) PackLds {
    unsigned short cum[64 * 18];         /* spectral models: cumulative frequencies */
    unsigned short tcum[18 + 144];       /* TNS order (2 x 9) and coefficient (8 x 18) models */
    unsigned char lut[4096];             /* context -> model */
    unsigned short bits[64 * 17];        /* bit cost (1/2048 bit) of a symbol under a model: the second quantisation's estimate (R/quantize_spec.c:60-170) */
    int pc[LC3D_PLAN_HEAD_WORDS];
};
extern __shared__ unsigned pack_fw[];    /* per wave: [16][64]: the lane's current 64-byte piece of its spectrum row */
typedef unsigned __attribute__((aligned(1), may_alias)) pk_u32u;

struct PkW { uint8_t* o; int nbytes; unsigned fw, bw; int q; int bp; unsigned low, range; int cache, carry, carry_count; bool wr; };   /* wr: the frame's bytes are stored (packed output: false where the frame does not fit) */
/* forward cursor: byte v (whole bytes from the range coder, single bits at finalisation) into byte bp if c, then advance.  Predicated rather than
 * branched: a lane-divergent `if` costs the scalar unit three to four instructions per nesting level, and the coder's renormalisation is four levels deep */
__device__ __forceinline__ void pk_emit(PkW& w, unsigned v, bool c)
{
    const bool in = c && w.bp < w.nbytes;
    const unsigned sh = (unsigned)(w.bp & 3) * 8u;
    w.fw |= in ? (v & 255u) << sh : 0u;
    if (in && sh == 24u) { if (w.wr) *(pk_u32u*)(w.o + (w.bp & ~3)) = w.fw; w.fw = 0; }
    w.bp += c ? 1 : 0;
}
__device__ __forceinline__ void pk_fwd_or(PkW& w, unsigned v) { if (w.bp < w.nbytes) w.fw |= (v & 255u) << ((w.bp & 3) * 8); }     /* finalisation only: OR without advancing */
/* backward cursor, R/enc_entropy.c:90-115: n (<= 32) bits of val, LSB first, appended at bit q of the reversed frame */
__device__ __forceinline__ void pk_back(PkW& w, unsigned val, int n)
{
    const int sh = w.q & 31;
    const unsigned long long acc = (unsigned long long)w.bw | ((unsigned long long)(n >= 32 ? val : val & ((1u << n) - 1u)) << sh);
    if (sh + n >= 32) {
        const int off = w.nbytes - 4 - 4 * (w.q >> 5);
        if (off >= 0 && w.wr) *(pk_u32u*)(w.o + off) = __builtin_bswap32((unsigned)acc);
        w.bw = (unsigned)(acc >> 32);
    } else w.bw = (unsigned)acc;
    w.q += n;
}
__device__ __forceinline__ void pk_bit_back(PkW& w, int bit) { pk_back(w, (unsigned)bit, 1); }
__device__ __forceinline__ void pk_uint_back(PkW& w, int val, int nbits) { pk_back(w, (unsigned)val, nbits); }
__device__ __forceinline__ void pk_shift(PkW& w, bool sact = true)  /* R/ari_codec.c:531-553, for the lanes with sact */
{
    const bool sh = sact && (w.low < 16711680u || w.carry == 1);
    pk_emit(w, (unsigned)(w.cache + w.carry), sh && w.cache >= 0);
    if (__any(sh && w.carry_count > 0)) {                                 /* pending 0xff bytes: rare */
        if (sh) while (w.carry_count > 0) { pk_emit(w, (unsigned)(w.carry + 255), true); w.carry_count--; }
    }
    w.cache = sh ? (int)(w.low >> 16) : w.cache;
    w.carry = sh ? 0 : w.carry;
    w.carry_count += (sact && !sh) ? 1 : 0;
    w.low = sact ? (w.low << 8) & 0xFFFFFFu : w.low;
}
__device__ __forceinline__ void pk_encode(PkW& w, unsigned freq, unsigned cum, bool act = true)       /* R/ari_codec.c:511-529, for the lanes with act */
{
    const unsigned r = w.range >> 10;
    const unsigned low = w.low + r * cum;
    w.carry = (act && (low >> 24) == 1) ? 1 : w.carry;
    w.low = act ? low & 0xFFFFFFu : w.low;
    w.range = act ? r * freq : w.range;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const bool s_ = act && w.range < 65536u;
        if (__any(s_)) { w.range = s_ ? w.range << 8 : w.range; pk_shift(w, s_); }
    }
}

/* R/adjust_global_gain.c:13-50 for one frame (per lane) */
__device__ __forceinline__ void lane_gain_adjust(const lc3d_plan* __restrict__ P, int f, int off, int& gg, int gg_min, float& gain, int target, int nBits, int& change)
{
    float delta;
    if (nBits < lc3t_gg_p1[f]) delta = (float)(((double)nBits + 48.0) / 16.0);
    else if (nBits < lc3t_gg_p2[f]) delta = ((float)nBits + lc3t_gg_d[f]) * lc3t_gg_c[f];
    else if (nBits < lc3t_gg_p3[f]) delta = (float)((double)nBits / 48.0);
    else delta = (float)((double)lc3t_gg_p3[f] / 48.0);
    delta = (float)round((double)delta);
    const int delta2 = (int)(delta + 2);
    change = 0;
    if (gg == 255 && nBits > target) change = 1;
    if ((gg < 255 && nBits > target) || (gg > 0 && nBits < target - delta2)) {
        if (nBits < target - delta2) gg = gg - 1;
        else if (gg == 254 || (float)nBits < (float)target + delta) gg = gg + 1;
        else gg = gg + 2;
        gg = imax(gg, gg_min - off);
        gain = P->gain_adj[gg + off + 256];
        change = 1;
    }
}

#ifndef PK_EU
#define PK_EU 4
#endif
#ifndef PK_HEAD_EU
#define PK_HEAD_EU 4
#endif
#ifndef PK_CODE_EU
#define PK_CODE_EU 6
#endif
/* MODE 0: head and coder in one kernel (lc3_enc_pack_kernel).  MODE 1 / 2: the two halves as kernels of their own (lc3_enc_pack_head_kernel leaves the frame's 56
 * parameters in the head of its scratch row, next to the quantised lines and residual words it leaves there anyway; lc3_enc_pack_code_kernel picks them up) - each half
 * with the registers IT needs: the head's 16-line rounds (lines, quantised lines, the next round in flight) against the coder's per-lane state machine. */
template <int MODE, bool PK = false> __device__ __forceinline__ void
pack_body(const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int* __restrict__ dump /* [cs][T][dstride] */, int dstride, int T, int tb, int nt, int ncs,
          uint8_t* __restrict__ out, int out_stride, uint8_t* __restrict__ status /* [cs][T] LC3D_ENC_ST_* bits, or null */,
          float* __restrict__ rows /* [cs][T][srow]: the shaped spectra of the pipelined path, or null: the record is complete (lc3_encode_kernel wrote it) */, int srow,
          const float* __restrict__ frec /* [cs][T][FR_WORDS] */, int skip_bytes /* channel-streams with frames of this size and more belong to lc3_enc_tailw_kernel; 0: none */,
          const long long* __restrict__ poff = nullptr /* PK: [stream][T] byte offset of each stream-frame in out, -1: not written (lc3_pack_offsets_kernel) */
#ifdef LC3_ENC_RPIPE
          , const int32_t* __restrict__ cnt = nullptr /* [stream] frames of each stream present in this call */
#endif
          )
{
    __shared__ PackLds L;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wpg = blockDim.x >> 6, tid = threadIdx.x, nthr = blockDim.x;
    if (MODE != 1) {
        for (int i = tid; i < 64 * 18; i += nthr) L.cum[i] = lc3t_ac_cum[i];
        for (int i = tid; i < 18; i += nthr) L.tcum[i] = lc3t_tns_order_cum[i];
        for (int i = tid; i < 144; i += nthr) L.tcum[18 + i] = lc3t_tns_coef_cum[i];
    }
    for (int i = tid; i < 4096 / 4; i += nthr) ((unsigned*)L.lut)[i] = ((const unsigned*)lc3t_ac_ctx_lut)[i];
    if (rows && MODE != 2) for (int i = tid; i < 64 * 17; i += nthr) L.bits[i] = lc3t_ac_bits[i];
    if (tid < LC3D_PLAN_HEAD_WORDS) L.pc[tid] = ((const int*)P)[tid];
    LSYNC();
#define KPI(f) uni(L.pc[offsetof(lc3d_plan, f) / 4])
    const int Lspec = KPI(ylen), channels = KPI(channels), fs = KPI(fs), hr = KPI(hrmode), bwb = KPI(bw_bits);
    const long long cf = ((long long)blockIdx.x * wpg + wv) * WAVE + lane;
    const bool inside = cf < (long long)ncs * nt;                                /* frames tb ... tb + nt - 1 of every channel-stream */
#ifdef LC3_ENC_RPIPE
    const bool valid_dense = inside && !(skip_bytes && chans[(int)(cf / nt)].nbytes >= skip_bytes);
#else
    const bool valid = inside && !(skip_bytes && chans[(int)(cf / nt)].nbytes >= skip_bytes);
#endif
#ifdef LC3_ENC_RPIPE                /* ragged: a lane whose frame is absent is not valid and shadows the wave's first present frame (lc3_kernels.hip: erp_shadow) - not frame
                                     * (0, tb), whose rows and records no kernel of this call may have written; a wave with no present frame is done */
    int cs = inside ? (int)(cf / nt) : 0, t = inside ? tb + (int)(cf % nt) : 0;
    const bool valid = valid_dense && t < cnt[cs / channels];
    if (!erp_shadow(valid, cs, t)) return;                                       /* (no barrier below) */
    const long long row = (long long)cs * T + t;
#define PK_ROW row
#else
    if (!__any(valid)) return;                                                   /* (no barrier below) */
    const int cs = valid ? (int)(cf / nt) : 0, t = valid ? tb + (int)(cf % nt) : 0;
    const long long row = (long long)cs * T + t;
#define PK_ROW (valid ? row : 0)
#endif
    const int strm = cs / channels;
    const lc3d_chan* C = &chans[cs];
    const int nbytes = valid ? C->nbytes : 0, total = C->total_bits, lpcw = C->lpc_weighting & 1;
    /* the frame's row of `dump`: plain rows when lc3_encode_kernel filled them, tiled like the spectrum rows (lc3_plan.h) when this kernel is its only user */
    const int RTd = rows ? T : 1;
    int* r = rows ? LC3D_ROW_BASE(dump, cs, t, T, dstride) : dump + PK_ROW * dstride;
#define RP(k_) (&r[LC3D_ROW_OFF((k_), RTd)])
    PkW w; w.o = out + ((size_t)strm * T + t) * out_stride + (valid ? C->out_off : 0); w.nbytes = nbytes; w.q = 0; w.fw = 0; w.bw = 0; w.wr = true;
    if (PK) { const long long po = valid ? poff[(size_t)strm * T + t] : -1; w.o = out + (po < 0 ? 0 : po) + (valid ? C->out_off : 0); w.wr = po >= 0; }
    unsigned* xb = pack_fw + (size_t)wv * PK_XBUF * WAVE;     /* a row is read in 64-byte pieces: each cache line is visited twice, not eight times */
    /* ---- parameters of the frame (isc[] of lc3_encode_kernel): the record head in 16-byte pieces, not one scattered load per field ---- */
    int rc[56];
    if (!rows || MODE == 2) {
#pragma unroll
        for (int i = 0; i < 56; i += 4) { const int4 v = *(const int4*)RP(i); rc[i] = v.x; rc[i + 1] = v.y; rc[i + 2] = v.z; rc[i + 3] = v.w; }
    } else {
        /* ======== the frame-parallel tail of the encoder, one frame per lane (R/enc_lc3_fl.c:123-141): gain adjustment, second quantisation with its
         * truncating bit count when the gain moved (R/adjust_global_gain.c, R/quantize_spec.c), noise level (R/noise_factor.c), residual bits
         * (R/residual_coding.c).  Every lane runs the reference's own scalar loops over its frame's spectrum row; the quantised lines go to the
         * lane's row of `dump` (the scratch the writer below reads back), nothing else leaves the registers. ======== */
#pragma unroll
        for (int i = 0; i < 56; i++) rc[i] = 0;
        float* xr = LC3D_ROW_BASE(rows, cs, t, T, srow);                        /* this frame's spectrum (tiled rows, lc3_plan.h) */
#define XP(k_) (&xr[LC3D_ROW_OFF((k_), T)])
        const int* fi = (const int*)(frec + PK_ROW * FR_WORDS);
        {   /* what the tail needs of the record: bandwidth, TNS / LTPF side bits, the rate kernel's four words; the coder's fields are fetched behind it */
            const int4 v = *(const int4*)&fi[FR_RATE];
            rc[I_GG] = v.x; rc[I_CHANGE] = v.y /* the gain's bits for a moment */; rc[I_NBITS] = v.z;
            rc[I_BW] = fi[FR_BWC]; rc[I_GGMIN] = (int)__int_as_float(fi[FR_GGMIN]);
            rc[I_TNS_BITS] = fi[FR_TNS + 3]; rc[I_LTPF_BITS] = fi[FR_LTPF + 3];
        }
        const int off = C->gg_off, fsi = KPI(fs_idx), dms = KPI(dms);
        const int tbq = C->target_bits_init - (rc[I_TNS_BITS] + rc[I_LTPF_BITS]);
        int gg = rc[I_GG], change; float gain = __int_as_float(rc[I_CHANGE]);
        const int nbits0 = rc[I_NBITS];
        lane_gain_adjust(P, fsi, off, gg, rc[I_GGMIN], gain, tbq, nbits0, change);
        if (!valid) change = 0;
        rc[I_GG] = gg; rc[I_CHANGE] = change;
        /* ---- pass 1: quantise (R/quantize_spec.c:37-47); for a frame whose gain moved, the bit count in coding order with its truncation
         *      point (:60-170, mode 0 / 1) ---- */
        const float offs = hr ? 0.5f : 0.375f, rgain = 1.0f / gain;
        const int half = Lspec >> 1;
        int rate1 = 0;
        if ((fs < 48000 && total > 320 + (fs / 8000 - 2) * 160) || (fs == 48000 && total > 800)) rate1 = 512;
        const bool m1 = change && ((fs < 48000 && total >= 640 + (fs / 8000 - 2) * 160) || (fs == 48000 && total >= 1120));    /* mode 1: LSBs may go uncoded */
        int cst = 0, nb = 0, nlsb = 0, snap_nb = 0, snap_nlsb = 0, lastnz1 = 1, lastnz2 = 2, nbits2 = 0;
        bool ovf = false;
        const int tgt2048 = tbq * 2048;
        /* The noise level (R/noise_factor.c:13-108) and the residual bits (R/residual_coding.c:13-75) ride in the same walk: both go over the quantised
         * lines in line order, and which lines the bit budget cuts off (R/quantize_spec.c:155-172: everything from the first tuple on whose running
         * count exceeds the target; the count only grows) is known tuple by tuple.  What is known only at the end - how many residual bits there is room
         * for - limits how many of the collected bits are used, not how they are formed.  (A second walk re-read the row and the quantised lines: 1 400 of
         * the kernel's 4 700 wave-cycles per frame, for 290 instructions.) */
        const int bw_bin = lc3t_bw_bins[KPI(bw_cls) * 6 + rc[I_BW]];
        const int width = dms == 100 ? 8 : 4, first = dms == 100 ? 24 : dms == 50 ? 12 : 6, hw = (width - 2) / 2;
        const unsigned wmask = (1u << (2 * hw + 1)) - 1u;
        int nz = 0, sumz = 0, nres = 0; float mean = 0;
        unsigned resw = 0, pfl = 0;                       /* pfl: flags of the non-zero lines of the round before */
        float xp0 = 0, xp1 = 0, xp2 = 0;                  /* its last three lines */
        /* A lane walks its own rows: 64-byte pieces (16 lines) per round, so that every cache line it touches is used in full by back-to-back
         * loads (single words per lane would fetch a line per word and lane, and 64 lanes x 4 waves do not fit the L1). */
        float4 xn[4];
#pragma unroll
        for (int j = 0; j < 4; j++) xn[j] = *(const float4*)XP(4 * j);      /* unconditional (a lane without a frame reads frame 0 of stream 0 and stores nothing): a select on a loaded register waits for the load on the spot */
        for (int k0 = 0; k0 < Lspec; k0 += 16) {                                  /* eight 2-tuples per round; the next round's lines are requested first */
            float xs[16];
#pragma unroll
            for (int j = 0; j < 4; j++) { xs[4 * j] = xn[j].x; xs[4 * j + 1] = xn[j].y; xs[4 * j + 2] = xn[j].z; xs[4 * j + 3] = xn[j].w; }
            if (k0 + 16 < Lspec) {
#pragma unroll
                for (int j = 0; j < 4; j++) xn[j] = *(const float4*)XP(k0 + 16 + 4 * j);
            }
            /* x / gain + offset, truncated (R/quantize_spec.c:37-47): by the reciprocal, and by the reference's division for a line whose
             * product lies that close to an integer (the same test as lc3_enc_rate_kernel's; a zero line gives +-offset -> 0 either way) */
            int q[16]; unsigned amb = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const float x = k0 + j < Lspec ? xs[j] : 0.0f;
                xs[j] = x;
                const float v = x * rgain + copysignf(offs, x);
                q[j] = (int)v;
                if (fabsf(v - rintf(v)) <= fabsf(v) * 5e-7f) amb |= 1u << j;
            }
            if (__any(amb != 0)) {
#pragma unroll
                for (int j = 0; j < 16; j++)
                    if ((amb >> j) & 1u) { const float x = xs[j]; q[j] = (int)truncf(x / gain + copysignf(offs, x)); }
            }
            if (valid) {
                if (hr) {
#pragma unroll
                    for (int j = 0; j < 4; j++) *(int4*)RP(PK_XQ + k0 + 4 * j) = make_int4(q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3]);
                } else {
                    int w_[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) { ovf |= q[2 * j] != (int)(int16_t)q[2 * j] || q[2 * j + 1] != (int)(int16_t)q[2 * j + 1]; w_[j] = (q[2 * j] & 0xFFFF) | (q[2 * j + 1] << 16); }
                    *(int4*)RP(PK_XQ + (k0 >> 1)) = make_int4(w_[0], w_[1], w_[2], w_[3]);
                    *(int4*)RP(PK_XQ + (k0 >> 1) + 4) = make_int4(w_[4], w_[5], w_[6], w_[7]);
                }
            }
            unsigned kp = valid ? 0xFFu : 0u;             /* tuples of this round that stay (a lane without a frame: none) */
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int k = k0 + 2 * j, x0 = q[2 * j], x1 = q[2 * j + 1];
                const bool nzt = (x0 | x1) != 0;
#ifndef PK_SKIP_BITS
                if (__any(change))
#else
                if (false)
#endif
                {
                    if (change && k < Lspec) {
                        int t = cst + rate1; if (k > half) t += 256;
                        int a = x0 < 0 ? -x0 : x0, b = x1 < 0 ? -x1 : x1;
                        if (!m1) nb += (imin(a, 1) + imin(b, 1)) * 2048;
                        int lev = 0;
                        while (imax(a, b) >= 4) {
                            nb += L.bits[L.lut[t + lev * 1024] * 17 + 16];
                            if (lev == 0 && m1) nlsb += 2; else nb += 2 * 2048;
                            a >>= 1; b >>= 1; lev = imin(lev + 1, 3);
                        }
                        nb += L.bits[L.lut[t + lev * 1024] * 17 + a + 4 * b];
                        if (m1) {
                            int am = x0 < 0 ? -x0 : x0, bm = x1 < 0 ? -x1 : x1;
                            if (lev > 0) { am >>= 1; bm >>= 1; if (am == 0 && x0 != 0) nlsb++; if (bm == 0 && x1 != 0) nlsb++; }
                            nb += (imin(am, 1) + imin(bm, 1)) * 2048;
                        }
                        if (nzt && nb <= tgt2048) { lastnz2 = k + 2; nbits2 = nb; }
                        if (k >= 2 && nb > tgt2048) kp &= ~(1u << j);       /* cut off by the bit budget (lines 0 and 1 always stay: lastnz starts at 2) */
                        lev = lev - 1;
                        const int tv = lev <= 0 ? 1 + (a + b) * (lev + 2) : 13 + lev;
                        cst = (cst & 15) * 16 + tv;
                    }
                }
                if (k == 0 || nzt) { if (k >= 2) lastnz1 = k + 1; snap_nb = nb; snap_nlsb = nlsb; }     /* the count as of the last coded tuple (k < lastnz) */
            }
#ifndef PK_SKIP_PASS2
            unsigned fl = 0;                              /* this round's lines that are coded non-zero; inside the bandwidth: the noise level's view */
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const bool nzl = q[j] != 0 && ((kp >> (j >> 1)) & 1u);
                fl |= (unsigned)(nzl && k0 + j < bw_bin) << j;
                if (nzl) {                                /* residual bit of this line (as many of them are used as there turns out to be room for) */
                    if (xs[j] >= (float)q[j] * gain) resw |= 1u << (nres & 31);
                    nres++;
                    if ((nres & 31) == 0) { *RP(PK_RES + (nres >> 5) - 1) = (int)resw; resw = 0; }
                }
            }
            /* noise level: lines k0 - 3 ... k0 + 12, whose neighbourhoods (hw <= 3 lines to either side) are known now.  Bit i of W = line k0 - 16 + i */
            {
                const unsigned W = pfl | (fl << 16);
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const int k = k0 - 3 + j;
                    if (k >= first && k < bw_bin && (W & (wmask << (13 + j - hw))) == 0) {
                        const float x = j == 0 ? xp0 : j == 1 ? xp1 : j == 2 ? xp2 : xs[j >= 3 ? j - 3 : 0];
                        nz++; sumz += k + 1; mean += fabsf(x / gain);
                    }
                }
                pfl = fl; xp0 = xs[13]; xp1 = xs[14]; xp2 = xs[15];
            }
#endif
        }
#ifndef PK_SKIP_PASS2
        {   /* the last three lines: nothing to their right */
            const unsigned W = pfl;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int k = ((Lspec + 15) & ~15) - 3 + j;
                if (k >= first && k < bw_bin && (W & (wmask << (13 + j - hw))) == 0) { nz++; sumz += k + 1; mean += fabsf((j == 0 ? xp0 : j == 1 ? xp1 : xp2) / gain); }
            }
        }
#endif
        if (status && ovf && valid) status[row] |= LC3D_ENC_ST_QUANT_RANGE;               /* R/quantize_spec.c:50 asserts this range */
        int lsb1 = 0, nb2;
        if (change) {
            int nbt = (snap_nb + 2047) >> 11; nb2 = (nbits2 + 2047) >> 11;
            if (m1) { nbt += snap_nlsb; nb2 += snap_nlsb; }
            lsb1 = (m1 && nbt > tbq) ? 1 : 0;
            rc[I_NBITS] = nbt;
        } else { lastnz2 = lastnz1 + 1; nb2 = nbits0; }
        rc[I_LASTNZ] = lastnz2; rc[I_LSB] = lsb1; rc[I_NBITS2] = nb2;
        const bool split = valid && nbytes <= 20 && dms == 100;
        const int mres = imax(lsb1 ? 0 : tbq - nb2 + 4 + (hr ? 10 : 0), 0);
        bool res_done = false;                            /* the residual words are complete as they stand */
        if (nres > mres) {                                /* more bits collected than there is room for: the word in progress goes out, the count is what fits */
            if (valid && (nres & 31)) *RP(PK_RES + (nres >> 5)) = (int)resw;
            nres = mres; res_done = true;
        }
        float fac = 0;
        if (sumz > 0) fac = mean / (float)nz;
        if (__any(split && nz > 0)) {
            if (split && nz > 0) {                    /* R/noise_factor.c:84-104: the zero lines in two groups around their mean position */
                const int msp = sumz / nz; float m1s = 0, m2s = 0; int j1 = 0;
                unsigned win = 0;
                for (int k = 0; k < bw_bin + hw; k++) {
                    int qv = 0;
                    if (k < bw_bin && k < lastnz2) { if (hr) qv = *RP(PK_XQ + k); else { const int w_ = *RP(PK_XQ + (k >> 1)); qv = (k & 1) ? (w_ >> 16) : ((w_ << 16) >> 16); } }
                    win = (win << 1) | (qv != 0 ? 1u : 0u);
                    const int kc = k - hw;
                    if (kc >= first && kc < bw_bin && (win & ((1u << (2 * hw + 1)) - 1u)) == 0) {
                        const float v = fabsf(*XP(kc)) / gain;
                        if (kc + 1 <= msp) { m1s += v; j1++; } else m2s += v;
                    }
                }
                const float n1 = m1s / (float)j1, n2 = m2s / (float)(nz - j1);
                fac = n1 < n2 ? n1 : n2;
            }
        }
        { float idx = (float)round((double)(8 - 16 * fac)); const float t_ = idx > 0 ? idx : 0; idx = t_ < 7 ? t_ : 7; rc[I_FACNS] = (int)idx; }
#ifdef PK_SKIP_HRSWEEP      /* diagnostic (tools/variants.sh): the output of such a build is not the encoder's */
        if (false) {
#else
        if (hr && __any(nres < mres && !lsb1)) {
#endif
            /* high-resolution mode: up to 19 more sweeps over the non-zero lines with a halved offset, on the refined spectrum (R/residual_coding.c:44-70).  Sixteen lines
             * (64 bytes of the row, 64 of the quantised lines) per step, like the walk above - line by line it was 4 bytes per lane and load, and a lane with few non-zero lines
             * (a silent stream: none) walked all of them nineteen times: 1.6 of the kernel's 2.7 ms on c96.  A sweep that finds no line to refine ends the lane's sweeps: nothing
             * changes any more, the reference's remaining sweeps are empty as well. */
            const bool sweeping = valid && !lsb1;
            float offset = .25f;
            {   /* sweep 0 has been counted above; redo it with the refinement written back */
                int n = 0;
                for (int k0 = 0; k0 < Lspec && __any(sweeping && n < mres && k0 < lastnz2); k0 += 16) {
                    if (sweeping && n < mres && k0 < lastnz2) {
                        int qv[16]; float xv[16];
#pragma unroll
                        for (int j = 0; j < 4; j++) { const int4 a = *(const int4*)RP(PK_XQ + k0 + 4 * j); qv[4 * j] = a.x; qv[4 * j + 1] = a.y; qv[4 * j + 2] = a.z; qv[4 * j + 3] = a.w;
                                                      const float4 b = *(const float4*)XP(k0 + 4 * j); xv[4 * j] = b.x; xv[4 * j + 1] = b.y; xv[4 * j + 2] = b.z; xv[4 * j + 3] = b.w; }
#pragma unroll
                        for (int j = 0; j < 16; j++) {
                            const int q1 = k0 + j < lastnz2 && k0 + j < Lspec ? qv[j] : 0;
                            if (q1 != 0 && n < mres) { const float x = xv[j]; xv[j] = x >= (float)q1 * gain ? x - gain * offset : x + gain * offset; n++; }
                        }
#pragma unroll
                        for (int j = 0; j < 4; j++) if (k0 + 4 * j < Lspec) *(float4*)XP(k0 + 4 * j) = make_float4(xv[4 * j], xv[4 * j + 1], xv[4 * j + 2], xv[4 * j + 3]);
                    }
                }
            }
            bool more = sweeping && nres < mres;
            for (int iter = 1; iter < 20 && __any(more); iter++) {
                offset *= .5f;
                const int before = nres;
                for (int k0 = 0; k0 < Lspec && __any(more && nres < mres && k0 < lastnz2); k0 += 16) {
                    if (more && nres < mres && k0 < lastnz2) {
                        int qv[16]; float xv[16];
#pragma unroll
                        for (int j = 0; j < 4; j++) { const int4 a = *(const int4*)RP(PK_XQ + k0 + 4 * j); qv[4 * j] = a.x; qv[4 * j + 1] = a.y; qv[4 * j + 2] = a.z; qv[4 * j + 3] = a.w;
                                                      const float4 b = *(const float4*)XP(k0 + 4 * j); xv[4 * j] = b.x; xv[4 * j + 1] = b.y; xv[4 * j + 2] = b.z; xv[4 * j + 3] = b.w; }
#pragma unroll
                        for (int j = 0; j < 16; j++) {
                            const int q1 = k0 + j < lastnz2 && k0 + j < Lspec ? qv[j] : 0;
                            if (q1 != 0 && nres < mres) {
                                const float x = xv[j];
                                if (x >= (float)q1 * gain) { resw |= 1u << (nres & 31); xv[j] = x - gain * offset; } else xv[j] = x + gain * offset;
                                nres++;
                                if ((nres & 31) == 0) { *RP(PK_RES + (nres >> 5) - 1) = (int)resw; resw = 0; }
                            }
                        }
#pragma unroll
                        for (int j = 0; j < 4; j++) if (k0 + 4 * j < Lspec) *(float4*)XP(k0 + 4 * j) = make_float4(xv[4 * j], xv[4 * j + 1], xv[4 * j + 2], xv[4 * j + 3]);
                    }
                }
                more = more && nres < mres && nres != before;
            }
        }
        if (valid && !res_done && (nres & 31)) *RP(PK_RES + (nres >> 5)) = (int)resw;
        rc[I_NRES] = nres;
        {   /* the coder's fields of the record: SNS indices, LTPF, TNS */
            int fw[FR_TNS + 20 - FR_IDX];
#pragma unroll
            for (int i = 0; i < FR_TNS + 20 - FR_IDX; i += 4) { const int4 v = *(const int4*)&fi[FR_IDX + i]; fw[i] = v.x; fw[i + 1] = v.y; fw[i + 2] = v.z; fw[i + 3] = v.w; }
#pragma unroll
            for (int i = 0; i < 7; i++) rc[I_SCF0 + i] = fw[i];
#pragma unroll
            for (int i = 0; i < 3; i++) rc[I_LTPF0 + i] = fw[FR_LTPF - FR_IDX + i];
#pragma unroll
            for (int i = 0; i < 20; i++) rc[I_TNS_NF + i] = fw[FR_TNS - FR_IDX + i];
        }
#undef XP
        if (MODE == 1) {                 /* the frame's parameters for lc3_enc_pack_code_kernel: the head of the scratch row */
            if (valid) {
#pragma unroll
                for (int i = 0; i < 56; i += 4) *(int4*)RP(i) = make_int4(rc[i], rc[i + 1], rc[i + 2], rc[i + 3]);
            }
            return;
        }
    }
#define r rc
    const int bw_idx = r[I_BW], lastnz = valid ? r[I_LASTNZ] : 0, lsbMode = r[I_LSB], gg = r[I_GG], fac_ns = r[I_FACNS], nres = r[I_NRES];
    const int nfilt = r[I_TNS_NF], ord0 = r[I_TNS_ORD0], ord1 = r[I_TNS_ORD1];
    const int lt0 = r[I_LTPF0], lt1 = r[I_LTPF1], lt2 = r[I_LTPF2];
    const int s0 = r[I_SCF0], s1 = r[I_SCF1], s2 = r[I_SCF2], s3 = r[I_SCF3], s4 = r[I_SCF4], s5 = r[I_SCF5], s6 = r[I_SCF6];
    if (valid) {
        /* ================= side information R/enc_entropy.c:25-87 ================= */
        if (bwb > 0) pk_uint_back(w, bw_idx, bwb);
        pk_uint_back(w, lastnz / 2 - 1, ilog2((unsigned)(Lspec / 2 - 1)) + 1);
        pk_bit_back(w, lsbMode);
        pk_uint_back(w, gg, 8);
        if (nfilt > 0) pk_bit_back(w, imin(1, ord0));
        if (nfilt > 1) pk_bit_back(w, imin(1, ord1));
        pk_bit_back(w, lt0);
        pk_uint_back(w, s0, 5); pk_uint_back(w, s1, 5);
        const int sub_msb = s2 >> 1, sub_lsb = s2 & 1, g_lsb = s3 & 1;
        pk_bit_back(w, sub_msb);
        pk_uint_back(w, s3 >> (s2 & 1), 1 + sub_msb);                    /* gain msbs: 1, 1, 2, 2 bits for sub-modes 0..3 */
        pk_bit_back(w, s4);
        if (sub_msb == 0) pk_uint_back(w, (sub_lsb == 0 ? s6 + 2 : g_lsb) * 2390004 + s5, 25);
        else pk_uint_back(w, sub_lsb != 0 ? 2 * s5 + g_lsb + 15158272 : s5, 24);
        if (lt0 == 1) { pk_uint_back(w, lt1, 1); pk_uint_back(w, lt2, 9); }
        pk_uint_back(w, fac_ns, 3);
    }
#undef r
    /* ================= range coder R/ari_codec.c:649-800 ================= */
    w.bp = 0; w.low = 0; w.range = 0xFFFFFFu; w.cache = -1; w.carry = 0; w.carry_count = 0;
#pragma unroll
    for (int f = 0; f < 2; f++) {
        const int ord = (valid && f < nfilt) ? (f ? ord1 : ord0) : 0;
        if (__any(ord > 0)) {
            { const int b = lpcw * 9 + imax(ord, 1); pk_encode(w, (unsigned)L.tcum[b] - L.tcum[b - 1], L.tcum[b - 1], ord > 0); }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (__any(j < ord)) {
                    const int b = 18 + j * 18 + (j < ord ? rc[I_TNS_IDX0 + f * 8 + j] : 0);
                    pk_encode(w, (unsigned)L.tcum[b + 1] - L.tcum[b], L.tcum[b], j < ord);
                }
            }
        }
    }
    /* ---- spectrum: every lane codes one symbol per step, whatever its own position ---- */
#define XW(k_) RP(PK_XQ + (k_))                        /* int16 pairs (one word per tuple), or int32 lines in high-resolution mode */
    int rate = 0;
    if ((fs < 48000 && total > 320 + (fs / 8000 - 2) * 160) || (fs == 48000 && total > 800)) rate = 512;
    int k = 0, lev = 0, c = 0, nl = 0;
    unsigned lsbw = 0;                               /* LSB-mode list: appended 32 bits at a time to the record's residual words */
    int x0 = 0, x1 = 0, a0 = 0, b0 = 0, maxlev = 0, nsh = 0, tctx = 0;
    bool fresh = true;
    const int rowlen = dstride - PK_XQ;
    int4 nx[4];
#pragma unroll
    for (int j = 0; j < 4; j++) nx[j] = *(const int4*)XW(4 * j);
    bool done = !valid || k >= lastnz;
#ifdef PK_SKIP_CODER      /* diagnostic builds (tools/variants.sh): instruction counts of the kernel's parts by leaving one out; the output of such a build is not the encoder's */
    done = true;
#endif
    /* The wave walks its rows piece by piece (16 words = 64 bytes per lane): the piece fetched one round ago goes to LDS and the
     * next one is requested for every lane at once - refilling per lane would run the refill code in almost every step, because
     * the lanes reach their piece boundaries at different steps.  Inside a piece the lanes run free. */
    for (int w0 = 0; __any(!done); w0 += PK_XBUF) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            xb[(4 * j + 0) * 64 + lane] = (unsigned)nx[j].x; xb[(4 * j + 1) * 64 + lane] = (unsigned)nx[j].y;
            xb[(4 * j + 2) * 64 + lane] = (unsigned)nx[j].z; xb[(4 * j + 3) * 64 + lane] = (unsigned)nx[j].w;
        }
        if (w0 + PK_XBUF < rowlen) {
#pragma unroll
            for (int j = 0; j < 4; j++) nx[j] = *(const int4*)XW(w0 + PK_XBUF + 4 * j);
        }
      const int wend = w0 + PK_XBUF;
      while (__any(!done && (hr ? k : k >> 1) < wend)) {
        if (!done && (hr ? k : k >> 1) < wend) {
            if (fresh) {                             /* a new tuple: values, escape count (R/quantize_spec.c:60-66 with its float log2), context */
                const int wi = hr ? k : k >> 1;                   /* word index in the row */
                if (hr) { x0 = (int)xb[(wi & (PK_XBUF - 1)) * 64 + lane]; x1 = (int)xb[((wi + 1) & (PK_XBUF - 1)) * 64 + lane]; }
                else { const int v = (int)xb[(wi & (PK_XBUF - 1)) * 64 + lane]; x0 = (v << 16) >> 16; x1 = v >> 16; }
                a0 = x0 < 0 ? -x0 : x0; b0 = x1 < 0 ? -x1 : x1;
                const int mx = imax(a0, b0);
                maxlev = mx == 0 ? -1 : flog2f_int((unsigned)imax(mx, 3)) - 1;
                nsh = mx >= 4 ? ilog2((unsigned)mx) - 1 : 0;
                tctx = c + rate; if (k > Lspec / 2) tctx += 256;
                lev = 0; fresh = false;
            }
            /* One coder symbol and up to two plain bits per step, the same instructions for both kinds of step: an escape (symbol 16 of
             * the model of its level class, then the two bits it shifts out) or the final symbol (then the signs).  A lane-divergent
             * if / else here ran both arms - two copies of the coder's renormalisation - in almost every step. */
            const bool esc = lev < maxlev;
            const int pki = L.lut[tctx + imin(esc ? lev : imax(maxlev, 0), 3) * 1024];
            const int af = a0 >> nsh, bf = b0 >> nsh;
            const int sym = esc ? 16 : af + 4 * bf;
            const unsigned cl = L.cum[pki * 18 + sym];
            pk_encode(w, (unsigned)L.cum[pki * 18 + sym + 1] - cl, cl);
            int a = a0, b = b0;
            if (lsbMode == 1) {                      /* LSB-mode list entries (R/ari_codec.c:735-757) */
                if (!esc && maxlev > 0) {
#define LSB_PUSH(bit_) do { lsbw |= (unsigned)(bit_) << (nl & 31); nl++; if ((nl & 31) == 0) { *RP(PK_RES + (nl >> 5) - 1) = (int)lsbw; lsbw = 0; } } while (0)
                    a >>= 1; LSB_PUSH(a0 & 1);
                    if (a == 0 && x0 != 0) LSB_PUSH(x0 < 0);
                    b >>= 1; LSB_PUSH(b0 & 1);
                    if (b == 0 && x1 != 0) LSB_PUSH(x1 < 0);
#undef LSB_PUSH
                }
            }
            const int sa = a != 0, sb = b != 0, ng0 = x0 < 0, ng1 = x1 < 0;
            const int nb = esc ? ((lsbMode == 1 && lev == 0) ? 0 : 2) : sa + sb;
            const int bv = esc ? (((a0 >> lev) & 1) | (((b0 >> lev) & 1) << 1)) : (sa ? (ng0 | (ng1 << 1)) : ng1);
            pk_back(w, (unsigned)bv, nb);
            const int levm = imin(nsh, 3) - 1;
            const int tv = levm <= 0 ? 1 + (af + bf) * (levm + 2) : 13 + levm;
            lev += esc;
            if (!esc) { c = (c & 15) * 16 + tv; k += 2; fresh = true; done = k >= lastnz; }
        }
      }
    }
    if (valid) {
        if (lsbMode == 1 && (nl & 31)) *RP(PK_RES + (nl >> 5)) = (int)lsbw;
        /* ---- residual / LSB bits R/ari_codec.c:764-797 ---- */
        const int bp_side = nbytes - 1 - (w.q >> 3), mask_log = w.q & 7;
        const int nbits_side = total - (8 * (bp_side + 1) + 8 - mask_log);
        int nbits_ari = (w.bp + 1) * 8 + 25 - flog2f_int(w.range);
        if (w.cache >= 0) nbits_ari += 8;
        if (w.carry_count > 0) nbits_ari += w.carry_count * 8;
        int nres_enc = total - (nbits_side + nbits_ari);
        if (nres_enc < 0 && status) status[row] |= LC3D_ENC_ST_BIT_BUDGET;         /* R/ari_codec.c:777 asserts this; here the frame is flagged */
        nres_enc = imin(nres_enc, lsbMode == 0 ? nres : nl);
        for (int k0 = 0; k0 < nres_enc; k0 += 32) {
            const unsigned wv2 = (unsigned)*RP(PK_RES + (k0 >> 5));
            const int cnt = imin(32, nres_enc - k0);
            pk_back(w, wv2, cnt);
        }
        /* ---- finalise R/ari_codec.c:573-647 ---- */
        int bits = 24 - flog2f_int(w.range);
        int mask = 0xFFFFFF >> bits, val = (int)w.low + mask; const int over1 = val >> 24;
        val &= 0xFFFFFF;
        int high = (int)w.low + (int)w.range; const int over2 = high >> 24;
        high &= 0xFFFFFF;
        val &= (0xFFFFFF - mask);
        if (over1 == over2) {
            if (val + mask >= high) { bits++; mask >>= 1; val = (((int)w.low + mask) & 0xFFFFFF) & (0xFFFFFF - mask); }
            if (val < (int)w.low) w.carry = 1;
        }
        w.low = (unsigned)val;
        int b = bits;
        if (bits > 8) { for (; b >= 1; b -= 8) pk_shift(w); } else pk_shift(w);
        bits = b; if (bits < 0) bits += 8;
        int last; const int nb = bits;
        if (w.carry_count > 0) {
            pk_emit(w, (unsigned)w.cache, true);
            for (int cc = w.carry_count; cc >= 2; cc--) pk_emit(w, 255u, true);
            last = (int)(255u << ((bits - 8) & 31));                    /* the reference's negative shift count, as x86 reduces it */
        } else last = w.cache;
        pk_fwd_or(w, (unsigned)last & (nb ? (0xFFu << (8 - nb)) & 0xFFu : 0u));      /* the top nb bits of `last` into byte bp */
        /* ---- the rest of the frame: the forward cursor's partial word (frame bytes f0 ...), the backward cursor's partial word (reversed
         * frame bytes 4 mb ... = frame bytes ... b1) and the unused bytes between them; a byte both cursors hold is OR-ed ---- */
        const int f0 = w.bp & ~3, mb = w.q >> 5, b1 = nbytes - 1 - 4 * mb;
        for (int i = f0; i <= b1; ) {
            if (i >= f0 + 4 && i + 7 <= b1) { if (w.wr) *(pk_u32u*)(w.o + i) = 0u; i += 4; continue; }
            const int fj = i - f0, bj = b1 - i;
            const unsigned v = (fj < 4 ? (w.fw >> (8 * fj)) & 255u : 0u) | (bj < 4 ? (w.bw >> (8 * bj)) & 255u : 0u);
            if (w.wr) w.o[i] = (uint8_t)v;
            i++;
        }
    }
#undef KPI
#undef RP
#undef XW
#undef PK_ROW
}
#define PK_ARGS const lc3d_plan* __restrict__ P, const lc3d_chan* __restrict__ chans, int* __restrict__ dump, int dstride, int T, int tb, int nt, int ncs, uint8_t* __restrict__ out, int out_stride, \
                uint8_t* __restrict__ status, float* __restrict__ rows, int srow, const float* __restrict__ frec, int skip_bytes
#define PK_PASS P, chans, dump, dstride, T, tb, nt, ncs, out, out_stride, status, rows, srow, frec, skip_bytes
#ifdef LC3_ENC_RPIPE      /* the ragged object: the two writers of the pipelined path's ragged calls, always with a table of offsets (the ragged plan kernel's slots, or the scan's) */
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(PK_EU, PK_EU))) lc3_enc_pack_kernel_pk_rag(PK_ARGS, const long long* __restrict__ poff LC3_ERP_OPT) { pack_body<0, true>(PK_PASS, poff, cnt); }
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(5, 5))) lc3_enc_pack_kernel_w5_pk_rag(PK_ARGS, const long long* __restrict__ poff LC3_ERP_OPT) { pack_body<0, true>(PK_PASS, poff, cnt); }
#else
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(PK_EU, PK_EU))) lc3_enc_pack_kernel(PK_ARGS) { pack_body<0>(PK_PASS); }
/* The same kernel under a 96-register budget (five waves per SIMD; 36 registers go to scratch).  The register file is what the call's kernels compete for (DESIGN.md
 * section 5), and 96-register waves pack with the rate kernel's: measured at 48 kHz / 10 ms, 4096 streams x 64 frames, Mframes/s with 128 / 96 registers - 40-byte frames
 * 104.4 / 111.0, 60: 106.8 / 115.1, 80 (c1): 105.4 / 111.4, 120: 91.7 / 91.1, 160: 88.4 / 88.1, 240: 82.0 / 82.3; calls of 16 / 32 frames at 80 bytes 93.2 / 91.0, 94.8 / 93.4;
 * c3 91.8 / 88.2, c4 116.7 / 116.1, c5 86.9 / 85.4, c96 32.2 / 32.1.  So: long calls of small frames (enc_launch). */
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(5, 5))) lc3_enc_pack_kernel_w5(PK_ARGS) { pack_body<0>(PK_PASS); }
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(PK_HEAD_EU, PK_HEAD_EU))) lc3_enc_pack_head_kernel(PK_ARGS) { pack_body<1>(PK_PASS); }
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(PK_CODE_EU, PK_CODE_EU))) lc3_enc_pack_code_kernel(PK_ARGS) { pack_body<2>(PK_PASS); }
/* packed output (lc3plus_enc_batch_encode_packed): the same four kernels, each frame at its offset of the call's table; every store stays inside the frame's
 * bytes (forward words at 4k < nbytes, backward words at nbytes - 4 - 4m >= 0, the rest bytewise up to nbytes - 1), so frames back to back do not overlap */
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(PK_EU, PK_EU))) lc3_enc_pack_kernel_pk(PK_ARGS, const long long* __restrict__ poff) { pack_body<0, true>(PK_PASS, poff); }
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(5, 5))) lc3_enc_pack_kernel_w5_pk(PK_ARGS, const long long* __restrict__ poff) { pack_body<0, true>(PK_PASS, poff); }
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(PK_HEAD_EU, PK_HEAD_EU))) lc3_enc_pack_head_kernel_pk(PK_ARGS, const long long* __restrict__ poff) { pack_body<1, true>(PK_PASS, poff); }
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(PK_CODE_EU, PK_CODE_EU))) lc3_enc_pack_code_kernel_pk(PK_ARGS, const long long* __restrict__ poff) { pack_body<2, true>(PK_PASS, poff); }
#endif
#undef PK_ARGS
#undef PK_PASS
