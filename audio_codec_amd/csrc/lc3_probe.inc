/* lc3_probe.inc -- the frame probe's kernels (included by lc3_probe.hip): the verdict of the bitstream parser on a frame, the reason where it refuses, and the
 * frame's side information, without decoding.  One item - a stream-frame, all its channels in order - per LANE, as lc3_dec_parse.inc maps the parser, and for
 * the same reason: the walk is serial inside a frame and reads nothing outside it.
 *
 * R = LC3plus_ETSI_src_v17171_20200723/src/floating_point.  lc3_probe_side_kernel: the side information (R/dec_entropy.c:120-270) from the last twelve bytes of
 * each channel, read straight from global memory; no LDS.  lc3_probe_full_kernel / _g: the side information, then the TNS symbols and the spectrum's tuples
 * exactly as R/ari_codec.c:204-509 walks them, keeping what a decision needs - the coder state, both read positions, the two-tuple context, the escape level -
 * and what the last record word (nres as the decoder ends with it) needs: the count of non-zero lines, and in LSB mode two bits per escaped tuple (which of its
 * lines are zero; the LSB pass reads a second bit for those).  No spectrum row, no second sweep, no SNS gains.  Frames of up to 128 bytes are staged in LDS
 * word-major, larger ones read through one cached word per reading direction (_g); models and context table in LDS, shared by the workgroup's waves.
 *
 * Reasons.  Each decision of the reference that returns records its own code; the three returns on the range decoder's ber flag record what set the flag
 * first (LC3P_REJ_*, lc3_probe_shim.h).  The parser only needs the decision and lets its symbol search run past the alphabet on an invalid coder state; here
 * the search ends on the last symbol as the reference's does, so that what follows the first error - which of two later checks fires - is the reference's too. */

struct __attribute__((aligned(16))) ProbeLds {
    unsigned short cum[64 * 32 + 8];     /* spectral models, 32 entries per model: 0 ... 1024 in [0, 17], 0xFFFF behind (lc3_launch.h ParseLds::cum) */
    unsigned short tcum[18 + 144];       /* TNS order (2 x 9) and coefficient (8 x 18) models */
    unsigned char lut[4096];             /* context -> model */
    int pc[LC3D_PLAN_HEAD_WORDS];
};
extern __shared__ unsigned probe_fw[];   /* per wave: [nw][64] frame words, word-major, then [nzw][64] zero flags of the escaped tuples (LSB mode), 2 bits each in tuple order */

#define QPI(f) uni(L.pc[offsetof(lc3d_plan, f) / 4])

/* A lane's frame bytes (as PLaneT of lc3_dec_parse.inc): staged in LDS (fw[word][lane]), or read from global memory through two one-word caches. */
template <bool GLOB> struct QLaneT { const unsigned* fw; int lane, nw, nbytes; const unsigned* g; int goff; int fwi, bwi; unsigned fwv, bwv; };
template <bool GLOB> __device__ __forceinline__ unsigned ql_gword(const QLaneT<GLOB>& p, int w)                 /* frame bytes 4w .. 4w+3 from global, zero from nbytes on */
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
template <bool GLOB> __device__ __forceinline__ unsigned ql_word_f(QLaneT<GLOB>& p, int w)
{
    if (!GLOB) { const bool ok = (unsigned)w < (unsigned)p.nw; const unsigned v = p.fw[(ok ? w : 0) * 64 + p.lane]; return ok ? v : 0u; }
    if (w != p.fwi) { p.fwv = ql_gword(p, w); p.fwi = w; }
    return p.fwv;
}
template <bool GLOB> __device__ __forceinline__ unsigned ql_word_b(QLaneT<GLOB>& p, int w)
{
    if (!GLOB) { const bool ok = (unsigned)w < (unsigned)p.nw; const unsigned v = p.fw[(ok ? w : 0) * 64 + p.lane]; return ok ? v : 0u; }
    if (w != p.bwi) { p.bwv = ql_gword(p, w); p.bwi = w; }
    return p.bwv;
}
/* (a byte index outside [0, nbytes) reads as zero) */
template <bool GLOB> __device__ __forceinline__ unsigned ql_fbyte(QLaneT<GLOB>& p, int i) { return i >= 0 ? (ql_word_f(p, i >> 2) >> ((i & 3) * 8)) & 255u : 0u; }
template <bool GLOB> __device__ __forceinline__ unsigned ql_byte(QLaneT<GLOB>& p, int i) { return i >= 0 ? (ql_word_b(p, i >> 2) >> ((i & 3) * 8)) & 255u : 0u; }
/* backward bit q = bit (q & 7) of byte nbytes - 1 - (q >> 3) */
template <bool GLOB> __device__ __forceinline__ int ql_bit(QLaneT<GLOB>& p, int q) { return (int)((ql_byte(p, p.nbytes - 1 - (q >> 3)) >> (q & 7)) & 1u); }

struct QAri { unsigned low, range; int bp, ber; };
/* one symbol of an n-symbol model whose cumulative frequencies start at cum[base] (R/ari_codec.c:47-118).  PAD32: the model's row holds 32 entries, 0xFFFF from
 * its total on, so the probes need no bound; on an invalid state (low >= (range >> 10) * 1024: ber) the reference's search stops at the last symbol, and so does
 * this one - with the bound in the plain form, by the fix-up behind the search in the padded one (n = 17 there) */
template <bool GLOB, bool PAD32> __device__ __forceinline__ int ql_symbol(QAri& st, QLaneT<GLOB>& p, const unsigned short* cum, int base, int n)
{
    const unsigned tmp = st.range >> 10;                 /* < 2^14: range stays below 2^24 */
    const bool inv = st.low >= (tmp << 10);
    if (inv) st.ber = 1;
    int s = 0;
    unsigned c0 = 0;
#pragma unroll
    for (int step = 16; step >= 1; step >>= 1) {
        const int c = s + step;
        if (PAD32) { const unsigned cc = cum[base + c]; if (st.low >= __umul24(tmp, cc)) { s = c; c0 = cc; } }
        else { const unsigned cc = cum[base + imin(c, n)]; if (c < n && st.low >= tmp * cc) { s = c; c0 = cc; } }
    }
    if (PAD32 && inv) { s = 16; c0 = cum[base + 16]; }
    const unsigned c1 = cum[base + s + 1];
    st.low -= __umul24(tmp, c0);                         /* both factors below 2^16 */
    st.range = __umul24(tmp, c1 - c0);
#pragma unroll
    for (int i = 0; i < 2; i++)
        if (st.range < 65536u) { st.low = ((st.low << 8) & 0xFFFFFFu) + ql_fbyte(p, st.bp < p.nbytes ? st.bp : -1); st.bp++; st.range <<= 8; }
    return s;
}

/* a record: LC3P_WORDS words, the used ones from registers, the rest zero.  body: words LC3P_BW ... LC3P_USED - 1, all zero unless the channel-frame is accepted */
__device__ __forceinline__ void probe_store(int32_t* __restrict__ r, int status, int reason, int nbytes, const int (&body)[LC3P_USED - LC3P_BW])
{
    r[LC3P_STATUS] = status; r[LC3P_REASON] = reason; r[LC3P_NBYTES] = nbytes;
#pragma unroll
    for (int i = LC3P_BW; i < LC3P_USED; i++) r[i] = status ? 0 : body[i - LC3P_BW];
#pragma unroll
    for (int i = LC3P_USED; i < LC3P_WORDS; i++) r[i] = 0;
}

/* the last LC3P_TAIL_BYTES bytes before `end` as lc3p_bits wants them, from the aligned words that hold them (all of them bytes of the channel: no frame is
 * shorter than 20 bytes) */
__device__ __forceinline__ void probe_tail_global(const uint8_t* __restrict__ end, unsigned& v0, unsigned& v1, unsigned& v2)
{
    const uint8_t* a = end - LC3P_TAIL_BYTES;
    const int sh = (int)(((size_t)a) & 3);
    const unsigned* w = (const unsigned*)(a - sh);
    unsigned a0 = w[0], a1 = w[1], a2 = w[2];
    if (sh) { const unsigned a3 = w[3]; a0 = (a0 >> (8 * sh)) | (a1 << (32 - 8 * sh)); a1 = (a1 >> (8 * sh)) | (a2 << (32 - 8 * sh)); a2 = (a2 >> (8 * sh)) | (a3 << (32 - 8 * sh)); }
    v0 = __builtin_bswap32(a2); v1 = __builtin_bswap32(a1); v2 = __builtin_bswap32(a0);
}

/* ================= SIDE depth: 256 items per workgroup, no LDS ================= */
extern "C" __global__ void __launch_bounds__(256)
lc3_probe_side_kernel(const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ dtab, int tab_n, const uint8_t* __restrict__ in, long long cap,
                      const long long* __restrict__ offs, const int32_t* __restrict__ nbs, int max_bytes, long long n_items, int32_t* __restrict__ info)
{
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_items) return;
    const int channels = P->channels, fs_idx = P->fs_idx, bwb = P->bw_bits, ylen = P->ylen, dms = P->dms;
    const int nb = nbs[id];
    const long long off = offs[id];
    const int cls = lc3p_item_class(nb, off, cap, max_bytes, dtab, tab_n, channels);
    bool refused = false;
    for (int ch = 0; ch < channels; ch++) {
        int32_t* r = info + ((size_t)id * channels + ch) * LC3P_WORDS;
        int rec[LC3P_WORDS];
#pragma unroll
        for (int i = 0; i < LC3P_WORDS; i++) rec[i] = 0;
        int status = 0, reason = 0, nbytes = 0;
        if (cls != LC3D_FRAME_GOOD) status = LC3P_ST_CONCEALED | (cls == LC3D_FRAME_LOST ? LC3P_ST_LOST : LC3P_ST_INVALID);
        else {
            nbytes = lc3p_chan_bytes(nb, channels, ch);
            if (refused) status = LC3P_ST_CONCEALED | LC3P_ST_SKIPPED;
            else {
                unsigned v0, v1, v2;
                int Q;
                probe_tail_global(in + off + lc3p_chan_off(nb, ch) + nbytes, v0, v1, v2);
                reason = lc3p_side(v0, v1, v2, fs_idx, bwb, ylen, dms, rec, &Q);
                if (reason) { status = LC3P_ST_CONCEALED; refused = true; }
            }
        }
        int body[LC3P_USED - LC3P_BW];
#pragma unroll
        for (int i = 0; i < LC3P_USED - LC3P_BW; i++) body[i] = rec[LC3P_BW + i];
        probe_store(r, status, reason, nbytes, body);
    }
}

/* ================= FULL depth ================= */
template <bool GLOB> __device__ __forceinline__ void
probe_full_body(const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ dtab, int tab_n, const uint8_t* __restrict__ in, long long cap,
                const long long* __restrict__ offs, const int32_t* __restrict__ nbs, int max_bytes, long long n_items,
                int nw_max /* LDS words staged per channel; 0: read from global memory */, int nzw /* LDS words of zero flags per lane */, int32_t* __restrict__ info)
{
    __shared__ ProbeLds L;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wpg = blockDim.x >> 6, tid = threadIdx.x, nthr = blockDim.x;
    for (int i = tid; i < 64 * 32 + 8; i += nthr) L.cum[i] = (i < 64 * 32 && (i & 31) < 18) ? lc3t_ac_cum[(i >> 5) * 18 + (i & 31)] : (unsigned short)0xFFFF;
    for (int i = tid; i < 18; i += nthr) L.tcum[i] = lc3t_tns_order_cum[i];
    for (int i = tid; i < 144; i += nthr) L.tcum[18 + i] = lc3t_tns_coef_cum[i];
    for (int i = tid; i < 4096 / 4; i += nthr) ((unsigned*)L.lut)[i] = ((const unsigned*)lc3t_ac_ctx_lut)[i];
    if (tid < LC3D_PLAN_HEAD_WORDS) L.pc[tid] = ((const int*)P)[tid];
    __syncthreads();
    const int Lspec = QPI(ylen), channels = QPI(channels), dms = QPI(dms), fs_idx = QPI(fs_idx), hr = QPI(hrmode), bwb = QPI(bw_bits);
    const long long id = ((long long)blockIdx.x * wpg + wv) * WAVE + lane;
    const bool valid = id < n_items;
    unsigned* fw = probe_fw + (size_t)wv * (nw_max + nzw) * WAVE;       /* this wave's slice; a lane only ever touches its own column */
    unsigned* zfl = fw + (size_t)nw_max * WAVE;
    const int max_lev = hr == 1 ? 13 + 8 : 13;
    const int nb = valid ? nbs[id] : 0;
    const long long off = valid ? offs[id] : 0;
    const int cls = valid ? lc3p_item_class(nb, off, cap, max_bytes, dtab, tab_n, channels) : LC3D_FRAME_LOST;
    const int fsz = cls == LC3D_FRAME_GOOD ? nb : 0;                    /* a lost or invalid item: no byte of it is read */
    bool refused = false;
    for (int ch = 0; ch < channels; ch++) {
        const int nbytes = fsz ? lc3p_chan_bytes(fsz, channels, ch) : 0;
        const int lpcw = dtab[nbytes].lpc_weighting;                    /* (entry 0 is zeroed) */
        const uint8_t* src = in + (fsz ? off + lc3p_chan_off(fsz, ch) : 0);
        /* ---- stage the channel's bytes: fw[w][lane], bytes from nbytes on are zero; whole words where the source is aligned and the frame has four bytes left ---- */
        {
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
        QLaneT<GLOB> p; p.fw = fw; p.lane = lane; p.nw = nw_max; p.nbytes = nbytes;
        p.goff = (int)(((size_t)src) & 3); p.g = (const unsigned*)(src - p.goff); p.fwi = -1; p.bwi = -1; p.fwv = 0; p.bwv = 0;
        int rec[LC3P_WORDS];
#pragma unroll
        for (int i = 0; i < LC3P_WORDS; i++) rec[i] = 0;
        /* ================= side information ================= */
        int Q = 0, why = 0;
        bool live = fsz != 0 && !refused;
        if (live) {
            unsigned v0 = 0, v1 = 0, v2 = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) { v0 |= ql_byte(p, nbytes - 1 - j) << (8 * j); v1 |= ql_byte(p, nbytes - 5 - j) << (8 * j); v2 |= ql_byte(p, nbytes - 9 - j) << (8 * j); }
            why = lc3p_side(v0, v1, v2, fs_idx, bwb, Lspec, dms, rec, &Q);
            if (why) live = false;
        }
        /* ================= TNS symbols, spectrum: R/ari_codec.c:204-509 ================= */
        int nres = 0;
        unsigned tp0 = 0, tp1 = 0, tp2 = 0;                       /* the 16 TNS coefficient indices, 5 bits each, six to a word */
        int ord[2] = {0, 0};
        if (__any(live)) {
            const int total_bits = 8 * nbytes, nfilt = rec[LC3P_NFILT], lsbMode = rec[LC3P_LSB], lastnz = live ? rec[LC3P_LASTNZ] : 0;
            const int rate = (fs_idx != 5 && total_bits > 160 + fs_idx * 160) ? 512 : 0;
            QAri st; st.low = 0; st.range = 0xFFFFFFu; st.bp = 0; st.ber = 0;
            for (int i = 0; i < 3; i++) { st.low = (st.low << 8) + ql_fbyte(p, st.bp < nbytes ? st.bp : -1); st.bp++; }
            int maxlag = 8; if (dms == 25) maxlag /= 2; if (dms == 50) maxlag /= 2;
            bool fail = !live;
            int ber_why = 0;                                       /* what set the ber flag first */
#pragma unroll
            for (int n = 0; n < 2; n++) {
                int o = (n < nfilt && !fail) ? rec[LC3P_TNS_ORDER + n] : 0;
                if (__any(o > 0)) {
                    {   /* lanes without this filter decode a copy of their state and drop it */
                        QAri s2 = st;
                        const int o2 = ql_symbol<GLOB, false>(s2, p, L.tcum, (lpcw & 1) * 9, 8) + 1;
                        if (o > 0) {
                            st = s2; o = o2;
                            if (st.ber && !ber_why) ber_why = LC3P_REJ_TNS_SYMBOL;
                            if (o > maxlag) { st.ber = 1; if (!ber_why) ber_why = LC3P_REJ_TNS_ORDER; }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        if (__any(k < o && !fail)) {
                            const bool on = k < o && !fail;
                            if (on && (nbytes - 1 - (Q >> 3)) < st.bp) { fail = true; why = LC3P_REJ_TNS_READER; }
                            QAri s2 = st;
                            const unsigned idv = (unsigned)ql_symbol<GLOB, false>(s2, p, L.tcum, 18 + k * 18, 17);
                            if (on && !fail) {
                                st = s2;
                                const int j = n * 8 + k;
                                if (j < 6) tp0 |= idv << (5 * j); else if (j < 12) tp1 |= idv << (5 * (j - 6)); else tp2 |= idv << (5 * (j - 12));
                                if (st.ber && !ber_why) ber_why = LC3P_REJ_TNS_SYMBOL;
                            }
                        }
                    }
                    if (o > 0 && !fail) ord[n] = o;
                }
            }
            if (!fail && st.ber > 0) { fail = true; why = ber_why; }
            /* ---- tuples: every lane decodes one symbol per step, whatever its own position ---- */
            int k = 0, lev = 0, xa = 0, xb = 0, c = 0, nnz = 0, nesc = 0;
            unsigned zacc = 0;                                     /* zero flags of up to sixteen escaped tuples, flushed to LDS word by word */
            bool done = fail || k >= lastnz;
            while (__any(!done)) {
                int tt = c + rate; if (k > Lspec / 2) tt += 256;
                const int pki = L.lut[(tt + imin(lev, 3) * 1024) & 4095];
                QAri s2 = st;
                const int sym = ql_symbol<GLOB, true>(s2, p, L.cum, pki * 32, 17);
                if (!done) {
                    st = s2;
                    if (st.ber && !ber_why) ber_why = LC3P_REJ_SPEC_SYMBOL;
                    bool fin = true;
                    if (sym == 16) {
                        if (lsbMode == 0 || lev > 0) { const int b0 = ql_bit(p, Q), b1 = ql_bit(p, Q + 1); Q += 2; xa += b0 << lev; xb += b1 << lev; }
                        lev++;
                        fin = lev > max_lev;
                    }
                    if (fin) {
                        if ((lev - 1) == 13 && sym == 16) { st.ber = 1; if (!ber_why) ber_why = LC3P_REJ_ESCAPE_14; }
                        if (hr == 0) lev = imin(lev, 13);
                        const int a = sym & 3, b = sym >> 2;
                        xa += a << lev; xb += b << lev;
                        if (lsbMode == 1 && lev > 0) {
                            zacc |= (unsigned)((xa == 0) | ((xb == 0) << 1)) << ((nesc & 15) * 2);
                            if (nzw > 0) zfl[imin(nesc >> 4, nzw - 1) * 64 + lane] = zacc;
                            nesc++;
                            if ((nesc & 15) == 0) zacc = 0;
                        }
                        nnz += (xa != 0) + (xb != 0);
                        Q += (xa > 0) + (xb > 0);                  /* the sign bits: the value is not needed */
                        const int lev1 = imin(lev, 3);
                        const int tn = lev1 <= 1 ? 1 + (a + b) * (lev1 + 1) : 12 + lev1;
                        c = (c & 15) * 16 + tn;
                        if (st.bp - (nbytes - 1 - (Q >> 3)) > 3) { fail = true; why = LC3P_REJ_OVERLAP; }
                        else if (st.ber > 0) { fail = true; why = ber_why; }
                        k += 2; lev = 0; xa = 0; xb = 0;
                        done = fail || k >= lastnz;
                    }
                }
            }
            if (!fail) {
                /* residual budget (R/ari_codec.c:405-409) */
                const int nbits_ari = (st.bp + 1 - 3) * 8 + 25 - flog2f_int(st.range);
                nres = total_bits - ((Q - 8) + nbits_ari);
                if (nres < 0) { fail = true; why = LC3P_REJ_NRES; }
            }
            if (!fail && lsbMode == 0) nres = imin(nres, hr ? nnz * 20 : nnz);
            /* ---- LSB mode: what the pass over the escaped tuples leaves of the budget (R/ari_codec.c:440-487) ---- */
            if (__any(!fail && lsbMode == 1)) {
                bool stop = fail || lsbMode != 1;
                for (int i = 0; __any(!stop && i < nesc); i++) {
                    if (!stop && i < nesc) {
                        const unsigned z = zfl[imin(i >> 4, imax(nzw, 1) - 1) * 64 + lane] >> ((i & 15) * 2);
#pragma unroll
                        for (int qq = 0; qq < 2; qq++) {
                            if (!stop && nres == 0) stop = true;
                            if (!stop) {
                                const int bit = ql_bit(p, Q); Q++; nres--;
                                if (bit == 1 && ((z >> qq) & 1u)) {
                                    if (nres == 0) stop = true;
                                    else { Q++; nres--; }
                                }
                            }
                        }
                    }
                }
            }
            if (fail) live = false;
        }
        if (valid) {
            int32_t* r = info + ((size_t)id * channels + ch) * LC3P_WORDS;
            int status = 0;
            if (cls != LC3D_FRAME_GOOD) status = LC3P_ST_CONCEALED | (cls == LC3D_FRAME_LOST ? LC3P_ST_LOST : LC3P_ST_INVALID);
            else if (refused) status = LC3P_ST_CONCEALED | LC3P_ST_SKIPPED;
            else if (!live) status = LC3P_ST_CONCEALED;
            rec[LC3P_TNS_ORDER] = ord[0]; rec[LC3P_TNS_ORDER + 1] = ord[1];
#pragma unroll
            for (int j = 0; j < 16; j++) rec[LC3P_TNS_IDX + j] = (int)(((j < 6 ? tp0 >> (5 * j) : j < 12 ? tp1 >> (5 * (j - 6)) : tp2 >> (5 * (j - 12)))) & 31u);
            rec[LC3P_NRES] = nres;
            int body[LC3P_USED - LC3P_BW];
#pragma unroll
            for (int i = 0; i < LC3P_USED - LC3P_BW; i++) body[i] = rec[LC3P_BW + i];
            probe_store(r, status, status == LC3P_ST_CONCEALED ? why : 0, nbytes, body);
        }
        if (fsz != 0 && !refused && !live) refused = true;
    }
}
#undef QPI

#define PROBE_FULL_KERNEL(name, GLOB) \
extern "C" __global__ void __launch_bounds__(4 * WAVE) \
name(const lc3d_plan* __restrict__ P, const lc3d_dchan* __restrict__ dtab, int tab_n, const uint8_t* __restrict__ in, long long cap, \
     const long long* __restrict__ offs, const int32_t* __restrict__ nbs, int max_bytes, long long n_items, int nw_max, int nzw, int32_t* __restrict__ info) \
{ probe_full_body<GLOB>(P, dtab, tab_n, in, cap, offs, nbs, max_bytes, n_items, nw_max, nzw, info); }
PROBE_FULL_KERNEL(lc3_probe_full_kernel, false)
PROBE_FULL_KERNEL(lc3_probe_full_kernel_g, true)
#undef PROBE_FULL_KERNEL
