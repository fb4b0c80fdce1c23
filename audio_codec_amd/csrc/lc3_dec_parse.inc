/* lc3_dec_parse.inc -- first decoder kernel: everything of a frame that is serial INSIDE the frame but carries no state from
 * frame to frame, mapped one stream-frame per LANE (included by lc3_kernels.hip; the other three kernels: lc3_dec_kernels.inc).
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  Stages (R/dec_lc3_fl.c:23-57): side information
 * (R/dec_entropy.c:120-270), TNS symbols + range decoder + sign / LSB bits (R/ari_codec.c:204-509), residual decoding
 * (R/residual_decoding.c:13-96), noise filling (R/noise_filling.c:13-80), global gain (R/apply_global_gain.c), the TNS
 * synthesis lattice (R/tns_decoder.c:13-51) and the SNS scale factors (R/sns_quantize_scf.c:432-544, R/sns_interpolate_scf.c:13-89).
 * All of them walk the spectrum or the bit stream in order - a wave-uniform loop would run them on one lane's worth of hardware -
 * but none of them reads anything of the previous frame, so the B x T frames of a launch are independent: a lane decodes one
 * stream-frame (all its channels, in order: a corrupt channel conceals the later ones, R/dec_lc3_fl.c:146-160) on its own, 64 frames
 * share one instruction stream.  What needs a wave (the transform) or the previous frame (overlap-add, LTPF) follows in the
 * other kernels.
 *
 * Data: frames of up to 128 bytes are staged in LDS word-major ([word][lane]: any per-lane word index is conflict-free), larger
 * ones are read from global memory through one cached word per reading direction (lc3_dec_parse_kernel_g); the spectral models
 * and the context table are gathered from LDS, shared by the workgroup's four waves; the spectrum of a lane lives in its own row
 * of a workspace in HBM ([channel-frame][480 or 960] words: int while parsing, float - in place - after the second sweep), written
 * and read in 32-byte pieces.  Side information and the 64 band gains go to a 112-word record per channel-frame (PR_* in
 * lc3_plan.h).  Arithmetic and operation order are those of the reference. */

/* PR_WORDS / PR_BFI / WS_ROW: lc3_plan.h */

extern __shared__ unsigned parse_fw[];   /* per wave: [nw][64] frame words, word-major, then [nlw][64] LSB-mode flags (bit (k / 2) of a lane's row is set when
                                          * tuple k had an escape level > 0) */

#define QPI(f) uni(L.pc[offsetof(lc3d_plan, f) / 4])

/* A lane's frame bytes.  Small frames are staged in LDS (fw[word][lane]); frames too large for four waves per workgroup are read
 * from global memory through two one-word caches, one per reading direction (both directions are monotone). */
template <bool GLOB> struct PLaneT { const unsigned* fw; int lane, nw, nbytes; const unsigned* g; int goff; int fwi, bwi; unsigned fwv, bwv; };
template <bool GLOB> __device__ __forceinline__ unsigned pl_gword(const PLaneT<GLOB>& p, int w)                 /* frame bytes 4w .. 4w+3 from global, zero from nbytes on */
{
    const int left = p.nbytes - 4 * w;
    if (w < 0 || left <= 0) return 0u;
    const int last = (p.goff + p.nbytes - 1) >> 2;                                  /* last aligned word that holds a byte of the frame */
    const unsigned lo = p.g[w];
    unsigned v = lo;
    if (p.goff) { const unsigned hi = w + 1 <= last ? p.g[w + 1] : 0u; v = (lo >> (8 * p.goff)) | (hi << (32 - 8 * p.goff)); }
    if (left < 4) v &= (1u << (8 * left)) - 1u;
    return v;
}
template <bool GLOB> __device__ __forceinline__ unsigned pl_word_f(PLaneT<GLOB>& p, int w)
{
    if (!GLOB) { const bool ok = (unsigned)w < (unsigned)p.nw; const unsigned v = p.fw[(ok ? w : 0) * 64 + p.lane]; return ok ? v : 0u; }      /* clamped and unconditional: a guarded LDS read is a divergent branch per byte */
    if (w != p.fwi) { p.fwv = pl_gword(p, w); p.fwi = w; }
    return p.fwv;
}
template <bool GLOB> __device__ __forceinline__ unsigned pl_word_b(PLaneT<GLOB>& p, int w)
{
    if (!GLOB) { const bool ok = (unsigned)w < (unsigned)p.nw; const unsigned v = p.fw[(ok ? w : 0) * 64 + p.lane]; return ok ? v : 0u; }
    if (w != p.bwi) { p.bwv = pl_gword(p, w); p.bwi = w; }
    return p.bwv;
}
/* (a negative byte index is a word index the staged read answers with zero) */
template <bool GLOB> __device__ __forceinline__ unsigned pl_fbyte(PLaneT<GLOB>& p, int i) { if (!GLOB) return (pl_word_f(p, i >> 2) >> ((i & 3) * 8)) & 255u; return i >= 0 ? (pl_word_f(p, i >> 2) >> ((i & 3) * 8)) & 255u : 0u; }
template <bool GLOB> __device__ __forceinline__ unsigned pl_byte(PLaneT<GLOB>& p, int i) { if (!GLOB) return (pl_word_b(p, i >> 2) >> ((i & 3) * 8)) & 255u; return i >= 0 ? (pl_word_b(p, i >> 2) >> ((i & 3) * 8)) & 255u : 0u; }
/* backward bit q = bit (q & 7) of byte nbytes - 1 - (q >> 3) */
template <bool GLOB> __device__ __forceinline__ int pl_bit(PLaneT<GLOB>& p, int q) { return (int)((pl_byte(p, p.nbytes - 1 - (q >> 3)) >> (q & 7)) & 1u); }
template <bool GLOB> __device__ __forceinline__ int pl_bits(PLaneT<GLOB>& p, int q, int n)          /* n <= 25 */
{
    const int b0 = p.nbytes - 1 - (q >> 3);
    const unsigned v = pl_byte(p, b0) | (pl_byte(p, b0 - 1) << 8) | (pl_byte(p, b0 - 2) << 16) | (pl_byte(p, b0 - 3) << 24);
    return (int)((v >> (q & 7)) & ((1u << n) - 1u));
}

struct PAri { unsigned low, range; int bp, ber; };
/* one symbol of an n-symbol model whose cumulative frequencies start at cum[base] (R/ari_codec.c:47-118) */
/* PAD32: the model's row holds 32 entries, 0xFFFF from its total on (ParseLds::cum): the probe needs neither a clamp nor a bound - on a state that is not valid
 * (low >= (range >> 10) * 1024: ber is set right here and the frame is concealed) the search may end beyond the alphabet, inside the row */
template <bool GLOB, bool PAD32 = false> __device__ __forceinline__ int pl_symbol(PAri& st, PLaneT<GLOB>& p, const unsigned short* cum, int base, int n)
{
    const unsigned tmp = st.range >> 10;                 /* < 2^14: range stays below 2^24 */
    if (st.low >= (tmp << 10)) st.ber = 1;
    int s = 0;
    unsigned c0 = 0;
#pragma unroll
    for (int step = 16; step >= 1; step >>= 1) {
        const int c = s + step;
        if (PAD32) { const unsigned cc = cum[base + c]; if (st.low >= __umul24(tmp, cc)) { s = c; c0 = cc; } }
        else { const unsigned cc = cum[base + imin(c, n)]; if (c < n && st.low >= tmp * cc) { s = c; c0 = cc; } }
    }
    const unsigned c1 = cum[base + s + 1];
    st.low -= __umul24(tmp, c0);                         /* both factors below 2^16 */
    st.range = __umul24(tmp, c1 - c0);
#pragma unroll
    for (int i = 0; i < 2; i++)
        if (st.range < 65536u) { st.low = ((st.low << 8) & 0xFFFFFFu) + pl_fbyte(p, st.bp < p.nbytes ? st.bp : -1); st.bp++; st.range <<= 8; }
    return s;
}

/* MPVQ de-indexing R/sns_quantize_scf.c:432-480 for one lane: m positions starting at pulses[OFF], k pulses */
template <int OFF, int MMAX> __device__ __forceinline__ void pl_pvq(const unsigned* offs, bool on, int k, int m, int ls_ind, int ind_, int (&pulses)[16])
{
    unsigned ind = (unsigned)ind_;
    int sign = 1 - 2 * ls_ind;
    bool done = !on;
#pragma unroll
    for (int pos = 0; pos < MMAX; pos++) {
        if (pos < m && !done) {
            int k_delta = 0;
            if (ind != 0) {
                const int row = (m - pos - 1) * 11;
                int idx = 0;
#pragma unroll
                for (int step = 8; step >= 1; step >>= 1) { const int c = idx + step; if (c <= k && c < 11 && ind >= offs[row + imin(c, 10)]) idx = c; }
                ind -= offs[row + idx];
                k_delta = k - idx;
            } else { pulses[OFF + pos] = sign * k; done = true; }
            if (!done && k_delta != 0) {
                pulses[OFF + pos] = sign * k_delta;
                sign = (ind % 2) != 0 ? -1 : 1;
                ind = ind / 2;
                k -= k_delta;
            }
        }
    }
}

/* Workgroup = up to four waves that share the model tables (7.5 KB); every wave owns a slice of the dynamic LDS.  VAR: per-frame sizes (a kernel of its own,
 * so that the fixed-size kernels stay the code they were). */
template <bool GLOB, bool VAR, bool PKD = false> __device__ __forceinline__ void
dec_parse_body(const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ chans, const uint8_t* __restrict__ in, int in_stride,
                     const uint8_t* __restrict__ bfi_flags /* [stream][T] or null */,
                     const uint16_t* __restrict__ sizes /* VAR: [stream][T] bytes of each stream-frame, 0 where lost */,
                     const lc3d_dchan* __restrict__ dtab /* VAR: configuration per channel byte count; otherwise chans[channel-stream] */,
                     int T, int n_streams, int nw_max /* LDS words staged per frame; 0: frames are read from global memory */,
                     int* __restrict__ rec /* [cs][T][PR_WORDS] */, float* __restrict__ ws /* [cs][T][wsr] */, int wsr /* words per spectrum row */,
                     const long long* __restrict__ offs = nullptr /* PKD: [stream][T] byte offset of each stream-frame in `in` (frames packed) */)
{
    __shared__ ParseLds L;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wpg = blockDim.x >> 6, tid = threadIdx.x, nthr = blockDim.x;
    for (int i = tid; i < 64 * 32 + 8; i += nthr) L.cum[i] = (i < 64 * 32 && (i & 31) < 18) ? lc3t_ac_cum[(i >> 5) * 18 + (i & 31)] : (unsigned short)0xFFFF;
    for (int i = tid; i < 18; i += nthr) L.tcum[i] = lc3t_tns_order_cum[i];
    for (int i = tid; i < 144; i += nthr) L.tcum[18 + i] = lc3t_tns_coef_cum[i];
    for (int i = tid; i < 4096 / 4; i += nthr) ((unsigned*)L.lut)[i] = ((const unsigned*)lc3t_ac_ctx_lut)[i];
    for (int i = tid; i < 176; i += nthr) L.mpvq[i] = lc3t_mpvq_offs[i];
    if (tid < LC3D_PLAN_HEAD_WORDS) L.pc[tid] = ((const int*)P)[tid];
    LSYNC();
    const int Lspec = QPI(ylen), channels = QPI(channels), dms = QPI(dms), fs_idx = QPI(fs_idx), hr = QPI(hrmode), bwb = QPI(bw_bits);
    const long long id = ((long long)blockIdx.x * wpg + wv) * WAVE + lane;
    const bool valid = id < (long long)n_streams * T;
    const int strm = valid ? (int)(id / T) : 0, t = valid ? (int)(id % T) : 0;
    int bfi = valid ? (bfi_flags ? (int)bfi_flags[(size_t)strm * T + t] : 0) : 1;
    const int nlw = (Lspec / 2 + 31) / 32;
    unsigned* fw = parse_fw + (size_t)wv * (nw_max + nlw) * WAVE;       /* this wave's slice; a lane only ever touches its own column */
    unsigned* lsbf = fw + (size_t)nw_max * WAVE;
    const int max_lev = hr == 1 ? 13 + 8 : 13;
    const int bwrow = (dms == 25 ? 0 : dms == 50 ? 1 : 2) * 6;

    /* VAR: a lane configures its channels from its own stream-frame size, split as R/dec_lc3_fl.c:148 does - at most two channels, the first
     * (fsz + 1) / 2 bytes, the second fsz / 2 behind it; the lanes of a wave may differ in every field of the configuration (they already do where a wave
     * spans two streams).  A lost frame comes with size 0: the zeroed configuration, which reads no byte of its slot (the concealment kernel gives it its
     * carried LTPF configuration). */
    for (int ch = 0; ch < channels; ch++) {
        const int cs = strm * channels + ch;
        const int fsz = VAR && valid ? (int)sizes[(size_t)strm * T + t] : 0;      /* (read again per channel: nothing of it stays live across the parse) */
        lc3d_dchan dc;
        { const int* s = (const int*)(VAR ? &dtab[(fsz + channels - 1 - ch) >> (channels - 1)] : &chans[valid ? cs : 0]); int* d = (int*)&dc;
#pragma unroll
          for (int i = 0; i < 8; i++) d[i] = s[i]; }
        if (VAR) dc.in_off = ch ? (fsz + 1) >> 1 : 0;
        const int nbytes = valid ? dc.nbytes : 0;
        /* ---- stage the frame bytes: fw[w][lane], bytes from nbytes on are zero ---- */
        {
            const uint8_t* src = (PKD ? in + (nbytes ? offs[(size_t)strm * T + t] : 0) : in + ((size_t)strm * T + t) * in_stride) + dc.in_off;
            const bool al = (((size_t)src) & 3) == 0;
            for (int w = 0; w < nw_max; w++) {             /* (nothing when the frames are read from global memory) */
                unsigned v = 0;
                const int left = nbytes - 4 * w;
                if (left >= 4 && al) v = ((const unsigned*)src)[w];
                else if (left > 0) {
#pragma unroll
                    for (int e = 0; e < 4; e++) if (e < left) v |= (unsigned)src[4 * w + e] << (8 * e);
                }
                fw[w * 64 + lane] = v;
            }
        }
        PLaneT<GLOB> p; p.fw = fw; p.lane = lane; p.nw = nw_max; p.nbytes = nbytes;
        {
            const uint8_t* src = (PKD ? in + (nbytes ? offs[(size_t)strm * T + t] : 0) : in + ((size_t)strm * T + t) * in_stride) + dc.in_off;
            p.goff = (int)(((size_t)src) & 3); p.g = (const unsigned*)(src - p.goff); p.fwi = -1; p.bwi = -1; p.fwv = 0; p.bwv = 0;
        }
        int* r = rec + ((size_t)cs * T + t) * PR_WORDS;
        /* spectrum rows are tiled like the encoder's (lc3_plan.h LC3D_ROW_BASE / _OFF): chunk c (16 words) of row (cs, t) at ((cs NCH + c) T + t) 16, so that the
         * 64 lanes of a wave - 64 consecutive frames of a stream - touch one contiguous run per access where they walk in step (the second sweep) */
        int* xrow = (int*)LC3D_ROW_BASE(ws, cs, t, T, wsr);
#define XR(k_) (xrow + LC3D_ROW_OFF((k_), T))
        int isc[40];
#pragma unroll
        for (int i = 0; i < 40; i++) isc[i] = 0;

        /* ================= side information R/dec_entropy.c:120-270 ================= */
        int Q = 0;
        if (bfi != 1) {
            int q = 0, bw = fs_idx;
            bool bad = false;
            if (bwb > 0) { bw = pl_bits(p, q, bwb); q += bwb; if (fs_idx < bw) bad = true; }
            const int nfilt = (bw < 3 || dms == 25) ? 1 : 2;
            const int nb = ilog2((unsigned)(Lspec / 2 - 1)) + 1;
            const int lastnz = (pl_bits(p, q, nb) + 1) * 2; q += nb;
            if (lastnz > Lspec) bad = true;
            const int lsb = pl_bit(p, q); q += 1;
            const int gg = pl_bits(p, q, 8); q += 8;
            int ord0 = pl_bit(p, q), ord1 = 0; q += 1;
            if (nfilt == 2) { ord1 = pl_bit(p, q); q += 1; }
            const int lt0 = pl_bit(p, q); q += 1;
            const int s0 = pl_bits(p, q, 5), s1 = pl_bits(p, q + 5, 5); q += 10;
            const int msb = pl_bit(p, q); q += 1;
            int s2 = msb * 2;
            int s3 = pl_bits(p, q, 1 + msb); q += 1 + msb;
            const int s4 = pl_bit(p, q); q += 1;
            int s5 = 0, s6 = 0, lsbm = 0;
            if (msb == 0) {
                const int tt = pl_bits(p, q, 25); q += 25;
                if (tt >= 33460056) bad = true;
                const int ind = tt / 2390004;
                s5 = tt - ind * 2390004;
                if (ind < 2) { lsbm = 1; s3 = s3 * 2 + ind; s6 = -2; } else { lsbm = 0; s6 = ind - 2; }
            } else {
                const int tt = pl_bits(p, q, 24); q += 24;
                if (tt >= 16708096) bad = true;
                if (tt >= 15158272) { lsbm = 1; s3 = s3 * 2 + ((tt - 15158272) & 1); s5 = (tt - 15158272) / 2; s6 = -2; } else { lsbm = 0; s5 = tt; s6 = -1; }
            }
            s2 += lsbm;
            int lt1 = 0, lt2 = 0;
            if (lt0 == 1) { lt1 = pl_bit(p, q); lt2 = pl_bits(p, q + 1, 9); q += 10; }
            const int fac = pl_bits(p, q, 3); q += 3;
            Q = q;
            /* the wave-per-stream version returns at the first failed check and leaves the later fields unread; nothing reads
             * them on a concealed frame, so only the decision matters here (checks in the reference's order are all "or"ed) */
            if (bad) bfi = 1;
            else {
                isc[0] = bw; isc[1] = lastnz; isc[2] = lsb; isc[3] = gg; isc[4] = nfilt; isc[5] = ord0; isc[6] = ord1;
                isc[23] = s0; isc[24] = s1; isc[25] = s2; isc[26] = s3; isc[27] = s4; isc[28] = s5; isc[29] = s6;
                isc[30] = lt0; isc[31] = lt1; isc[32] = lt2; isc[33] = fac;
            }
        }

        /* ================= TNS symbols, spectrum: R/ari_codec.c:204-509 ================= */
        int nres = 0, res_present = 0, nnz = 0, sdacc = 0;
        if (__any(bfi != 1)) {
            const bool live0 = bfi != 1;
            const int total_bits = 8 * nbytes, nfilt = isc[4], lsbMode = isc[2], lastnz = live0 ? isc[1] : 0;
            const int rate = (fs_idx != 5 && total_bits > 160 + fs_idx * 160) ? 512 : 0;
            PAri st; st.low = 0; st.range = 0xFFFFFFu; st.bp = 0; st.ber = 0;
            for (int i = 0; i < 3; i++) { st.low = (st.low << 8) + pl_fbyte(p, st.bp < nbytes ? st.bp : -1); st.bp++; }
            int maxlag = 8; if (dms == 25) maxlag /= 2; if (dms == 50) maxlag /= 2;
            bool fail = !live0;
#pragma unroll
            for (int n = 0; n < 2; n++) {
                int ord = (n < nfilt && !fail) ? isc[5 + n] : 0;
                if (__any(ord > 0)) {
                    {   /* lanes without this filter decode a copy of their state and drop it */
                        PAri s2 = st;
                        const int o2 = pl_symbol(s2, p, L.tcum, (dc.lpc_weighting & 1) * 9, 8) + 1;
                        if (ord > 0) { st = s2; ord = o2; if (ord > maxlag) st.ber = 1; }
                    }
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        if (__any(k < ord && !fail)) {
                            const bool on = k < ord && !fail;
                            if (on && (nbytes - 1 - (Q >> 3)) < st.bp) fail = true;
                            PAri s2 = st;
                            const int idv = pl_symbol(s2, p, L.tcum, 18 + k * 18, 17);
                            if (on && !fail) { st = s2; isc[7 + n * 8 + k] = idv; }
                        }
                    }
                    if (ord > 0 && !fail) isc[5 + n] = ord;
                }
            }
            if (st.ber > 0) fail = true;
            /* ---- tuples: every lane decodes one symbol per step, whatever its own position ---- */
            for (int i = 0; i < nlw; i++) lsbf[i * 64 + lane] = 0;
            int k = 0, lev = 0, xa = 0, xb = 0, c = 0;
            int grp[8];                               /* the four most recent tuples: stored as one 32-byte group (bins 8m .. 8m + 7) */
#pragma unroll
            for (int i = 0; i < 8; i++) grp[i] = 0;
            bool done = fail || k >= lastnz;
            while (__any(!done)) {
                int tt = c + rate; if (k > Lspec / 2) tt += 256;
                const int pki = L.lut[(tt + imin(lev, 3) * 1024) & 4095];
                PAri s2 = st;
                const int sym = pl_symbol<GLOB, true>(s2, p, L.cum, pki * 32, 17);
                if (!done) {
                    st = s2;
                    bool fin = true;
                    if (sym == 16) {
                        if (lsbMode == 0 || lev > 0) { const int b0 = pl_bit(p, Q), b1 = pl_bit(p, Q + 1); Q += 2; xa += b0 << lev; xb += b1 << lev; }
                        lev++;
                        fin = lev > max_lev;
                    }
                    if (fin) {
                        if ((lev - 1) == 13 && sym == 16) st.ber = 1;
                        if (hr == 0) lev = imin(lev, 13);
                        if (lsbMode == 1 && lev > 0) lsbf[(k >> 6) * 64 + lane] |= 1u << ((k >> 1) & 31);
                        const int a = sym & 3, b = sym >> 2;
                        xa += a << lev; xb += b << lev;
                        nnz += (xa != 0) + (xb != 0);
                        sdacc += xa * k + xb * (k + 1);
                        if (xa > 0) { if (pl_bit(p, Q) == 1) xa = -xa; Q++; }
                        if (xb > 0) { if (pl_bit(p, Q) == 1) xb = -xb; Q++; }
                        const int slot = (k >> 1) & 3, kbase = k & ~7;
#pragma unroll
                        for (int sl = 0; sl < 4; sl++) if (slot == sl) { grp[2 * sl] = xa; grp[2 * sl + 1] = xb; }
                        const int lev1 = imin(lev, 3);
                        const int tn = lev1 <= 1 ? 1 + (a + b) * (lev1 + 1) : 12 + lev1;
                        c = (c & 15) * 16 + tn;
                        if (st.bp - (nbytes - 1 - (Q >> 3)) > 3) fail = true;
                        if (st.ber > 0) fail = true;
                        k += 2; lev = 0; xa = 0; xb = 0;
                        done = fail || k >= lastnz;
                        if (!fail && (slot == 3 || done)) {           /* bins of the group beyond the last tuple are zero, as are all bins after it */
                            *(int4*)XR(kbase) = make_int4(grp[0], grp[1], grp[2], grp[3]);
                            *(int4*)XR(kbase + 4) = make_int4(grp[4], grp[5], grp[6], grp[7]);
#pragma unroll
                            for (int i = 0; i < 8; i++) grp[i] = 0;
                        }
                    }
                }
            }
            if (!fail) {
                /* residual budget (R/ari_codec.c:405-409) */
                const int nbits_ari = (st.bp + 1 - 3) * 8 + 25 - flog2f_int(st.range);
                nres = total_bits - ((Q - 8) + nbits_ari);
                if (nres < 0) fail = true;
            }
            if (!fail && lsbMode == 0) { nres = imin(nres, hr ? nnz * 20 : nnz); res_present = 1; }
            /* ---- LSB mode: the saved least significant bits, in tuple order, while the budget lasts (R/ari_codec.c:440-487) ---- */
            if (__any(!fail && lsbMode == 1)) {
                bool stop = fail || lsbMode != 1;
                for (int kk = 0; kk < Lspec; kk += 2) {
                    if (!__any(!stop && kk < lastnz)) break;
                    if (!stop && kk < lastnz && ((lsbf[(kk >> 6) * 64 + lane] >> ((kk >> 1) & 31)) & 1u)) {
                        int2 v2 = *(int2*)XR(kk);
                        int vv[2] = {v2.x, v2.y};
#pragma unroll
                        for (int qq = 0; qq < 2; qq++) {
                            if (!stop && nres == 0) stop = true;
                            if (!stop) {
                                int bit = pl_bit(p, Q); Q++; nres--;
                                if (bit == 1) {
                                    int v = vv[qq];
                                    if (v > 0) { v++; sdacc += kk + qq; }
                                    else if (v < 0) { v--; sdacc += kk + qq; }
                                    else if (nres == 0) stop = true;
                                    else {
                                        bit = pl_bit(p, Q); Q++; nres--;
                                        v = bit == 0 ? 1 : -1;
                                        sdacc += kk + qq;
                                    }
                                    vv[qq] = v;
                                }
                            }
                        }
                        *(int2*)XR(kk) = make_int2(vv[0], vv[1]);
                    }
                }
            }
            if (fail) bfi = 1;
            else {
                isc[34] = nres; isc[35] = res_present; isc[36] = Q;
                int sd = sdacc & 65535; if (sd >= 32768) sd -= 65536;
                isc[37] = sd;
                isc[38] = 0;
            }
        }
        /* the seed sums |x| * i: the accumulator above used signed values before the sign was applied (xa, xb >= 0 there) */

        /* ================= second sweep over the lane's spectrum: residual, noise filling, gain, TNS ================= */
        if (__any(bfi != 1)) {
            const bool live = bfi != 1;
            const int2 x01 = *(int2*)XR(0);
            const int zf = (isc[1] == 2 && x01.x == 0 && x01.y == 0 && isc[3] == 0 && isc[33] == 7);
            if (live) isc[38] = zf;
            const int bw_stop = lc3t_bw_bins[bwrow + (live ? isc[0] : 0)];
            const int tw = dms == 100 ? 3 : 1, so = dms == 100 ? 24 : dms == 50 ? 12 : 6;
            const float fac = (float)((8.0 - (double)isc[33]) / 16.0);
            int seed = isc[37];
            const float g = P->gain_adj[(live ? isc[3] + dc.gg_off : 0) + 256];
            const int nresv = isc[34], Qr = isc[36], resp = live ? isc[35] : 0;
            const int nnz_tot = nnz;
            const bool nofill = !live || zf != 0;
            /* TNS set-up (R/tns_decoder.c:13-51) */
            const int nfilt = live ? isc[4] : 0;
            const int start = (600 * (live ? dc.N_red_tns : 1) * 2 / (live ? dc.fs_red_tns : 1)) + 1;
            const int o0 = nfilt > 0 ? isc[5] : 0, o1 = nfilt > 1 ? isc[6] : 0;
            /* 1-based bin ranges of the two filters */
            const int a0 = start, e0 = nfilt == 2 ? bw_stop / 2 : bw_stop, a1 = bw_stop / 2 + 1, e1 = bw_stop;
            float rc0[8], rc1[8], stt[9];
#pragma unroll
            for (int j = 0; j < 8; j++) { rc0[j] = lc3t_tns_rc_pts[isc[7 + j] & 31]; rc1[j] = lc3t_tns_rc_pts[isc[15 + j] & 31]; }
#pragma unroll
            for (int j = 0; j < 9; j++) stt[j] = 0;
            float rca[8]; int orda = o0;                 /* the active filter: coefficients (zero from its order on) and order */
#pragma unroll
            for (int j = 0; j < 8; j++) rca[j] = j < o0 ? rc0[j] : 0.0f;
            const int lz8 = live ? (isc[1] + 7) & ~7 : 0;   /* the row holds bins [0, lz8); everything after is zero and was never written */
            int nidx = 0;                            /* index of the next non-zero line among the non-zero lines */
            /* sliding window of the integer spectrum: xi[j] = x[k - 3 + j], j = 0..6 */
            int win[7];
#pragma unroll
            for (int j = 0; j < 7; j++) win[j] = 0;
            {
                const int4 f0 = *(int4*)XR(0);
                win[3] = f0.x; win[4] = f0.y; win[5] = f0.z; win[6] = f0.w;     /* x[0..3]; refilled below */
            }
            /* the same window as flags for the noise filling: bit j = line k - 3 + j is non-zero and below the bandwidth's last line (a line from there on never counts,
             * R/noise_filling.c:27-40: the window ends at min(bw_stop - 1, k + tw)), so that "all zero around k" is one masked test instead of seven compares with their bounds */
            const int flim = imin(lz8, bw_stop);
            unsigned nzf = 0;
#pragma unroll
            for (int j = 3; j < 7; j++) nzf |= (unsigned)(win[j] != 0 && j - 3 < flim) << j;
            const unsigned nzm = tw == 3 ? 0x7Fu : 0x1Cu;                       /* lines k - tw ... k + tw */
            /* both pieces a step needs were requested a step earlier (the second one used to be requested by the step that reads it: once the step's own
             * work was cut down, that wait was what a wave spent its time on) */
            int4 nxa = *(int4*)XR(4), nxb = make_int4(0, 0, 0, 0);
            if (8 < wsr) nxb = *(int4*)XR(8);
            for (int k0 = 0; k0 < Lspec; k0 += 8) {                               /* 32 bytes in, 32 bytes out per lane and step */
                const int4 cur = nxa;                                             /* x[k0+4 .. k0+7] */
                const int4 cur2 = nxb;                                            /* x[k0+8 .. k0+11] */
                nxa = make_int4(0, 0, 0, 0); nxb = make_int4(0, 0, 0, 0);
                if (k0 + 12 < wsr) nxa = *(int4*)XR(k0 + 12);
                if (k0 + 16 < wsr) nxb = *(int4*)XR(k0 + 16);
                const int ahead[8] = {cur.x, cur.y, cur.z, cur.w, cur2.x, cur2.y, cur2.z, cur2.w};
                float outv[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int k = k0 + u;
                    const int xi = win[3];
                    float v = (float)xi;
                    /* residual decoding R/residual_decoding.c:13-96: line j of the non-zero lines owns bits j, j + nnz, j + 2 nnz ... */
                    if (resp && xi != 0) {
                        if (hr) {
                            float offset = 0.25f;
                            for (int it = 0; it < 20; it++) {
                                const int n = it * nnz_tot + nidx;
                                if (n >= nresv) break;
                                const int bit = pl_bit(p, Qr + n);
                                v = bit == 0 ? v - offset : v + offset;
                                offset = offset / 2;
                            }
                        } else if (nidx < nresv) {
                            const int bit = pl_bit(p, Qr + nidx);
                            if (bit == 0) v = v > 0 ? v - 0.1875f : v - 0.3125f;
                            else v = v > 0 ? v + 0.3125f : v + 0.1875f;
                        }
                        nidx++;
                    }
                    /* noise filling R/noise_filling.c:13-80 */
                    if (!nofill && k >= so && k < bw_stop) {
                        if ((nzf & nzm) == 0) {
                            seed = (13849 + (seed + 32768) * 31821) & 65535; seed -= 32768;
                            v = seed >= 0 ? fac : -fac;
                        }
                    }
                    /* global gain */
                    v = v * g;
                    /* TNS synthesis lattice: bin m = k + 1 */
                    {
                        const int m = k + 1;
                        const bool sw = o1 > 0 && m == a1;              /* the second filter takes over: its coefficients become the active ones (the state runs on) */
                        if (__any(sw)) {
#pragma unroll
                            for (int l = 0; l < 8; l++) rca[l] = sw ? (l < o1 ? rc1[l] : 0.0f) : rca[l];
                            orda = sw ? o1 : orda;
                        }
                        const bool in0 = o0 > 0 && m >= a0 && m <= e0, in1 = o1 > 0 && m >= a1 && m <= e1;
                        if (in0 || in1) {
                            /* taps from the order on have a zero coefficient: s - 0 * st is s (the states are finite), so only the state update needs the order */
                            float sv = v;
#pragma unroll
                            for (int l = 7; l >= 0; l--) {
                                sv = sv - rca[l] * stt[l];
                                if (l < 7) stt[l + 1] = l < orda - 1 ? rca[l] * sv + stt[l] : stt[l + 1];
                            }
                            stt[0] = sv;
                            v = sv;
                        }
                    }
                    outv[u] = k < Lspec ? v : 0.0f;
                    /* slide the window */
#pragma unroll
                    for (int j = 3; j < 6; j++) win[j] = win[j + 1];
                    win[6] = (k + 4 < lz8) ? ahead[u] : 0;
                    nzf = (nzf >> 1) | ((unsigned)(ahead[u] != 0 && k + 4 < flim) << 6);
                }
                if (live) { *(float4*)XR(k0) = make_float4(outv[0], outv[1], outv[2], outv[3]); *(float4*)XR(k0 + 4) = make_float4(outv[4], outv[5], outv[6], outv[7]); }
            }
        }
        isc[PR_BFI] = bfi;
        if (valid) {
#pragma unroll
            for (int i = 0; i < 40; i += 4) *(int4*)&r[i] = make_int4(isc[i], isc[i + 1], isc[i + 2], isc[i + 3]);
        }
        /* ================= SNS scale factors -> 64 band gains (R/sns_quantize_scf.c:482-544, R/sns_interpolate_scf.c:13-89) ================= */
        if (__any(bfi != 1)) {
            const bool live = bfi != 1;
            float* gq = (float*)(r + PR_GAINS);
            const int s0 = isc[23] & 31, s1 = isc[24] & 31, submode = isc[25] & 3, s3 = isc[26] & 7, s4 = isc[27], s5 = isc[28], s6 = isc[29];
            int pulses[16];
#pragma unroll
            for (int i = 0; i < 16; i++) pulses[i] = 0;
            pl_pvq<0, 16>(L.mpvq, live, submode < 2 ? 10 : submode == 2 ? 8 : 6, submode < 2 ? 10 : 16, s4, s5, pulses);
            pl_pvq<10, 6>(L.mpvq, live && submode == 0, 1, 6, s6 % 2, s6 / 2, pulses);
            float sum = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) sum += (float)(pulses[i] * pulses[i]);
            sum = sqrtf(sum);
            float vv[16], g[16];
#pragma unroll
            for (int i = 0; i < 16; i++) vv[i] = (float)pulses[i] / sum;
            const float gain = lc3t_sns_dec_gains[submode * 8 + s3];
            const float n1 = __int_as_float(uni(L.pc[offsetof(lc3d_plan, c_idct_n1) / 4])), n2 = __int_as_float(uni(L.pc[offsetof(lc3d_plan, c_idct_n2) / 4]));
#pragma unroll
            for (int i = 0; i < 16; i++) {
                float acc = 0;
#pragma unroll
                for (int j = 0; j < 16; j++) { float tt = (float)((double)vv[j] * P->idct_cos[i * 16 + j]); if (j == 0) tt *= n2; acc += tt; }
                const float vi = n1 * acc;
                const float st1 = i < 8 ? lc3t_sns_lf[s0 * 8 + i] : lc3t_sns_hf[s1 * 8 + i - 8];
                g[i] = st1 + vi * gain;
            }
            /* interpolation to 64 bands; the values go through the record so that the band merge below can index them */
            if (live) {
                float gint[4];
#pragma unroll
                for (int b = 0; b < 64; b++) {
                    float v;
                    if (b < 2) v = g[0];
                    else if (b < 62) {
                        const int n = (b - 2) >> 2, rr = (b - 2) & 3;
                        const double dd = (double)(g[n + 1] - g[n]);
                        v = (float)((double)g[n] + (double)(2 * rr + 1) * dd / 8.0);
                    } else {
                        const double dd = (double)(g[15] - g[14]);
                        v = b == 62 ? (float)((double)g[15] + dd / 8.0) : (float)((double)g[15] + 3.0 * dd / 8.0);
                    }
                    gint[b & 3] = v;
                    if ((b & 3) == 3) *(float4*)&gq[b - 3] = make_float4(gint[0], gint[1], gint[2], gint[3]);
                }
            }
            const int nbd = QPI(nbands);
            const int d = 64 - nbd;
            const float ratio = fabsf((float)(1.0 - 32.0 / (double)(float)nbd));
            const int n4 = (int)round((double)(ratio * (float)nbd));
            for (int b = 0; b < nbd; b++) {
                if (live) {
                    float v;
                    if (nbd == 64) v = gq[b];
                    else if (d < 32) v = b < d ? (float)((double)(gq[2 * b] + gq[2 * b + 1]) / 2.0) : gq[b + d];
                    else if (b < n4) v = (float)((double)(gq[4 * b] + gq[4 * b + 1] + gq[4 * b + 2] + gq[4 * b + 3]) / 4.0);
                    else { const int i = b - n4; v = (float)((double)(gq[4 * n4 + 2 * i] + gq[4 * n4 + 2 * i + 1]) / 2.0); }
                    gq[b] = m_powf(2.0f, v);
                }
            }
        }
    }
}

#undef XR
/* frames staged in LDS (up to 128 bytes); frames read from global memory (nw_max = 0); each with one size per channel-stream (chans) or with
 * per-frame sizes (_var) */
#ifndef DEC_PARSE_EU
#define DEC_PARSE_EU 4
#endif
#define DEC_PARSE_KERNEL(name, GLOB, VAR) \
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(DEC_PARSE_EU, DEC_PARSE_EU))) \
name(const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ chans, const uint8_t* __restrict__ in, int in_stride, \
     const uint8_t* __restrict__ bfi_flags, const uint16_t* __restrict__ sizes, const lc3d_dchan* __restrict__ dtab, int T, int n_streams, int nw_max, \
     int* __restrict__ rec, float* __restrict__ ws, int wsr) \
{ dec_parse_body<GLOB, VAR>(P, chans, in, in_stride, bfi_flags, sizes, dtab, T, n_streams, nw_max, rec, ws, wsr); }
DEC_PARSE_KERNEL(lc3_dec_parse_kernel, false, false)
DEC_PARSE_KERNEL(lc3_dec_parse_kernel_g, true, false)
DEC_PARSE_KERNEL(lc3_dec_parse_kernel_var, false, true)
DEC_PARSE_KERNEL(lc3_dec_parse_kernel_g_var, true, true)
#undef DEC_PARSE_KERNEL
/* frames packed back to back (lc3plus_dec_batch_decode_packed): the per-frame-size kernels addressing each stream-frame through the offset table.  Only good
 * frames are read (a lost or invalid one has size 0: nbytes 0), and only the aligned words that hold a byte of the frame (the staged read takes whole words
 * where the source is aligned and the frame has four bytes left, bytes otherwise; pl_gword stops at the last word holding a frame byte). */
#define DEC_PARSE_KERNEL_PK(name, GLOB) \
extern "C" __global__ void __launch_bounds__(4 * WAVE) __attribute__((amdgpu_waves_per_eu(DEC_PARSE_EU, DEC_PARSE_EU))) \
name(const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ chans, const uint8_t* __restrict__ in, const long long* __restrict__ offs, \
     const uint8_t* __restrict__ bfi_flags, const uint16_t* __restrict__ sizes, const lc3d_dchan* __restrict__ dtab, int T, int n_streams, int nw_max, \
     int* __restrict__ rec, float* __restrict__ ws, int wsr) \
{ dec_parse_body<GLOB, true, true>(P, chans, in, 0, bfi_flags, sizes, dtab, T, n_streams, nw_max, rec, ws, wsr, offs); }
DEC_PARSE_KERNEL_PK(lc3_dec_parse_kernel_var_pk, false)
DEC_PARSE_KERNEL_PK(lc3_dec_parse_kernel_g_var_pk, true)
#undef DEC_PARSE_KERNEL_PK
