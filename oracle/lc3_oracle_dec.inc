/* lc3_oracle_dec.inc -- TEST INFRASTRUCTURE (part of the CPU oracle, included by lc3_oracle.c).
 *
 * Scalar restatement of the ETSI float DECODER (R/dec_lc3_fl.c and its callees; R = LC3plus_ETSI_src_v17171_20200723/
 * src/floating_point) in the reference's operation order, including its packet-loss concealment (noise substitution,
 * R/plc_noise_substitution0.c).  Pinned against the compiled reference by tests/test_oracle_vs_ref.py (decoded PCM, sample for
 * sample).  It is the oracle of the decoder row of SURVEY 8(f); nothing in the product links it. */

#define LC3O_LTPF_Y 880                 /* ceil(228 * 48000 / 12800) + 6 = 861 <= 880 */

typedef struct {
    /* size-derived: R/setup_dec_lc3.c:188-299 */
    int last_size, targetBytes, total_bits, lpc_weighting, gg_off, N_red_tns, fs_red_tns, ltpf_beta_idx; float ltpf_beta;
    /* cross-frame state */
    float imdct_mem[LC3O_MAX_N];
    float ltpf_mem_x[16], ltpf_mem_y[LC3O_LTPF_Y];
    int ltpf_mem_pitch_int, ltpf_mem_pitch_fr, ltpf_mem_beta_idx, ltpf_param_mem[3]; float ltpf_mem_gain;
    float q_d_prev[LC3O_MAX_N]; int nbLost, prevBfi, prevprevBfi, plc_seed; float cum_alpha;
    int last_reject;                    /* LC3O_REJ_* of the last frame: why the bitstream was refused, 0 for a decoded or flagged frame */
} dchan_t;

struct lc3o_dec {
    int fs, fs_out, fs_idx, channels, dms, hrmode; float frame_ms;
    int N, ylen, la, nbands, bw_bits;
    const float* win; const uint16_t* bands; const uint16_t* cut_bins;
    cpx tw1[LC3O_MAX_N / 2], tw2[LC3O_MAX_N / 2]; float dct4_norm;
    double idct_cos[16][16];
    lc3o_dec_trace* trace;
    dchan_t ch[LC3O_MAX_CH];
};

int lc3o_dec_sizeof(void) { return (int)sizeof(lc3o_dec); }
void lc3o_dec_set_trace(lc3o_dec* d, lc3o_dec_trace* tr) { d->trace = tr; }

/* R/setup_dec_lc3.c:71-185 set_dec_frame_params */
static void dec_frame_params(lc3o_dec* d)
{
    if (d->fs_idx == 5) d->hrmode = 1;
    d->N = d->fs / 100;
    d->ylen = d->hrmode == 1 ? d->N : IMIN(400, d->N);
    if (d->dms == 25) { d->N >>= 2; d->ylen /= 4; }
    if (d->dms == 50) { d->N >>= 1; d->ylen /= 2; }
    d->bw_bits = d->hrmode ? 0 : lc3t_bw_bits[d->fs_idx];
    const int cls = d->dms == 25 ? 0 : d->dms == 50 ? 1 : 2;
    d->cut_bins = &lc3t_bw_bins[cls * 6];
    const lc3t_cfg_t* c = find_cfg(d->fs_idx, d->dms, d->hrmode);
    d->win = NULL; d->bands = NULL; d->nbands = 64; d->la = 0;
    if (c) { d->win = &lc3t_win_pool[c->win_off]; d->bands = &lc3t_band_pool[c->band_off]; d->nbands = c->nbands; d->la = c->la_zeros; }
    const int len = d->N;
    for (int i = 0; i < len / 2; i++) { d->tw1[i] = cexpi_f(-M_PI * (i + 0.25) / len); d->tw2[i] = cexpi_f(-M_PI * i / len); }
    d->dct4_norm = 1.0 / sqrtf(len / 2);
    for (int i = 0; i < 16; i++) for (int j = 0; j < 16; j++)
        d->idct_cos[i][j] = cos(M_PI / (2.0 * (float)16) * (2.0 * ((float)i + 1.0) - 1.0) * ((float)j));
    for (int ch = 0; ch < d->channels; ch++) {
        dchan_t* s = &d->ch[ch];
        s->ltpf_mem_beta_idx = -1;
        s->cum_alpha = 1; s->plc_seed = 24607;
    }
}

int lc3o_dec_init(lc3o_dec* d, int samplerate, int channels)           /* R/lc3.c:238-245, R/setup_dec_lc3.c:33-69 */
{
    if (!d) return LC3O_NULL_ERROR;
    int ok = 0; { static const int rates[] = {8000, 16000, 24000, 32000, 44100, 48000, 96000}; for (unsigned i = 0; i < 7; i++) ok |= rates[i] == samplerate; }
    if (!ok) return LC3O_SAMPLERATE_ERROR;
    if (channels < 1 || channels > LC3O_MAX_CH) return LC3O_CHANNELS_ERROR;
    memset(d, 0, sizeof *d);
    d->fs = samplerate == 44100 ? 48000 : samplerate; d->fs_out = samplerate;
    d->fs_idx = d->fs == 96000 ? 5 : d->fs == 48000 ? 4 : d->fs / 8000 - 1;     /* FS2FS_IDX, R/defines.h */
    d->channels = channels; d->frame_ms = 10; d->dms = 100;
    dec_frame_params(d);
    return 0;
}
int lc3o_dec_set_frame_ms(lc3o_dec* d, float ms)                        /* R/lc3.c:254-263 */
{
    if (!d) return LC3O_NULL_ERROR;
    const int dms = (int)ceil(ms * 10);
    if (dms != 25 && dms != 50 && dms != 100) return LC3O_FRAMEMS_ERROR;
    d->frame_ms = ms; d->dms = dms;
    dec_frame_params(d);
    return 0;
}
int lc3o_dec_set_hrmode(lc3o_dec* d, int hr)                            /* R/lc3.c:347-356 */
{
    if (!d) return LC3O_NULL_ERROR;
    if (d->fs_idx < 4 && hr != 0) return LC3O_SAMPLERATE_ERROR;
    if (d->fs_idx == 5 && hr == 0) return LC3O_HRMODE_ERROR;
    d->hrmode = hr > 0;
    dec_frame_params(d);
    return 0;
}
int lc3o_dec_get_output_samples(const lc3o_dec* d) { return d ? d->N : 0; }
int lc3o_dec_last_reject(const lc3o_dec* d, int ch) { return d && ch >= 0 && ch < d->channels ? d->ch[ch].last_reject : 0; }
int lc3o_dec_reject_count(void) { return LC3O_REJ_COUNT; }
const char* lc3o_dec_reject_name(int code)
{
    static const char* const names[LC3O_REJ_COUNT] = {"none", "bandwidth", "lastnz", "sns_index_25", "sns_index_24", "tns_order", "tns_reader", "tns_symbol",
                                                      "overlap", "spec_symbol", "escape_14", "nres"};
    return code >= 0 && code < LC3O_REJ_COUNT ? names[code] : "";
}
/* a `return 1` records its own code; one that follows the range decoder's ber flag records what set the flag first (BER) */
#define LC3O_REJECT(code) do { *why = (code); } while (0)
#define LC3O_BER(code) do { if (!ber_why) ber_why = (code); } while (0)

/* R/setup_dec_lc3.c:188-299 update_dec_bitrate */
static int dec_bitrate(lc3o_dec* d, dchan_t* s, int nbytes)
{
    int minB = 20, maxB = 400;
    if (d->hrmode) {
        if (d->dms == 25) { maxB = 210; minB = d->fs == 48000 ? 54 : d->fs == 96000 ? 62 : -1; }
        else if (d->dms == 50) { maxB = 375; minB = d->fs == 48000 ? 93 : d->fs == 96000 ? 109 : -1; }
        else { maxB = 625; minB = d->fs == 48000 ? 156 : d->fs == 96000 ? 187 : -1; }
        if (minB < 0) return LC3O_HRMODE_ERROR;
    }
    if (nbytes < minB || nbytes > maxB) return LC3O_NUMBYTES_ERROR;
    s->targetBytes = nbytes; s->total_bits = nbytes << 3;
    s->lpc_weighting = s->total_bits < 480;
    s->gg_off = -(IMIN(115, s->total_bits / (10 * (d->fs_idx + 1))) + 105 + 5 * (d->fs_idx + 1));
    int totalBits = s->total_bits;
    if (d->frame_ms == 2.5) { s->lpc_weighting = s->total_bits < 120; totalBits = s->total_bits * 4.0 * (1.0 - 0.4); }
    if (d->frame_ms == 5) { s->lpc_weighting = s->total_bits < 240; totalBits = s->total_bits * 2 - 160; }
    if (d->N > 40 * ((float)d->dms / 10.0)) { s->N_red_tns = 40 * ((float)d->dms / 10.0); s->fs_red_tns = 40000; }
    else { s->N_red_tns = d->N; s->fs_red_tns = d->fs; }
    const int b = totalBits, o = (d->fs_idx - 1) * 80;
    if (b < 400 + o) { s->ltpf_beta = 0.4; s->ltpf_beta_idx = 0; }
    else if (b < 480 + o) { s->ltpf_beta = 0.35; s->ltpf_beta_idx = 1; }
    else if (b < 560 + o) { s->ltpf_beta = 0.3; s->ltpf_beta_idx = 2; }
    else if (b < 640 + o) { s->ltpf_beta = 0.25; s->ltpf_beta_idx = 3; }
    else { s->ltpf_beta = 0; s->ltpf_beta_idx = -1; }
    if (d->hrmode == 1) { s->ltpf_beta = 0; s->ltpf_beta_idx = -1; }
    return 0;
}

/* backward bit reader: R/dec_entropy.c:16-43 */
typedef struct { const uint8_t* p; int bp, mask; } bitr;
static int rd_bit(bitr* r) { const int b = (r->p[r->bp] & r->mask) ? 1 : 0; if (r->mask == 128) { r->mask = 1; r->bp--; } else r->mask *= 2; return b; }
static int rd_uint(bitr* r, int n) { int v = rd_bit(r); for (int i = 1; i < n; i++) v += rd_bit(r) << i; return v; }

/* R/dec_entropy.c:120-270.  Returns 1 when the frame has to be concealed. */
static int dec_side(const lc3o_dec* d, const uint8_t* bytes, int nbytes, bitr* r, int* gg, int* scf_idx, int* fac_ns, int* nfilt, int* tns_order,
                    int* ltpf, int* bw, int* lastnz, int* lsb, int* why)
{
    r->p = bytes; r->bp = nbytes - 1; r->mask = 1;
    if (d->bw_bits > 0) { *bw = rd_uint(r, d->bw_bits); if (d->fs_idx < *bw) { LC3O_REJECT(LC3O_REJ_BANDWIDTH); return 1; } } else *bw = d->fs_idx;
    *nfilt = (*bw < 3 || d->dms == 25) ? 1 : 2;
    *lastnz = (rd_uint(r, (int)ceil(m_log2f(d->ylen / 2))) + 1) * 2;
    if (*lastnz > d->ylen) { LC3O_REJECT(LC3O_REJ_LASTNZ); return 1; }
    *lsb = rd_bit(r);
    *gg = rd_uint(r, 8);
    for (int i = 0; i < *nfilt; i++) tns_order[i] = rd_bit(r);
    ltpf[0] = rd_bit(r);
    scf_idx[0] = rd_uint(r, 5); scf_idx[1] = rd_uint(r, 5);
    const int msb = rd_bit(r);
    static const int gbits[4] = {1, 1, 2, 2};
    scf_idx[2] = msb * 2;
    scf_idx[3] = rd_uint(r, gbits[scf_idx[2]]);
    scf_idx[4] = rd_bit(r);
    int lsbm = 0;
    if (msb == 0) {
        const int t = rd_uint(r, 25);
        if (t >= 33460056) { LC3O_REJECT(LC3O_REJ_SNS_INDEX_25); return 1; }
        const int ind = t / 2390004;
        scf_idx[5] = t - ind * 2390004;
        if (ind < 2) { lsbm = 1; scf_idx[3] = scf_idx[3] * 2 + ind; scf_idx[6] = -2; } else { lsbm = 0; scf_idx[6] = ind - 2; }
    } else {
        const int t = rd_uint(r, 24);
        if (t >= 16708096) { LC3O_REJECT(LC3O_REJ_SNS_INDEX_24); return 1; }
        if (t >= 15158272) { lsbm = 1; scf_idx[3] = scf_idx[3] * 2 + ((t - 15158272) & 1); scf_idx[5] = (t - 15158272) / 2; scf_idx[6] = -2; }
        else { lsbm = 0; scf_idx[5] = t; scf_idx[6] = -1; }
    }
    scf_idx[2] += lsbm;
    if (ltpf[0] == 1) { ltpf[1] = rd_bit(r); ltpf[2] = rd_uint(r, 9); } else { ltpf[1] = 0; ltpf[2] = 0; }
    *fac_ns = rd_uint(r, 3);
    return 0;
}

/* range decoder: R/ari_codec.c:47-118 */
typedef struct { uint32_t low, range; int bp, ber; const uint8_t* p; } adec;
static int ad_decode(adec* st, const uint16_t* cum /* cum[0..n], cum[n] = 1024 */, int n)
{
    const int tmp = (int)(st->range >> 10);
    if (st->low >= (uint32_t)(tmp << 10)) st->ber = 1;
    int val = n - 1;
    while (st->low < (uint32_t)(tmp * cum[val])) val--;
    st->low -= (uint32_t)(tmp * cum[val]);
    st->range = (uint32_t)(tmp * (cum[val + 1] - cum[val]));
    while (st->range < 65536) { st->low = (int)(((unsigned)st->low << 8) & 0xFFFFFFu) + st->p[st->bp]; st->bp++; st->range <<= 8; }
    return val;
}

/* R/ari_codec.c:204-509.  Returns 1 when the frame has to be concealed. */
static int dec_spectrum(const lc3o_dec* d, const dchan_t* s, const uint8_t* bytes, bitr* r, int nfilt, int lsbMode, int lastnz, int* tns_order, int fac_ns,
                        int gg, uint8_t* resBits, int* x, int* nf_seed, int* tns_idx, int* zero_frame, int* nres, int* res_present, int* why)
{
    const int L = d->ylen, total_bits = 8 * s->targetBytes;
    int rate = 0;
    if (d->fs_idx != 5 && total_bits > 160 + d->fs_idx * 160) rate = 512;
    adec st; st.p = bytes; st.low = 0; st.range = 0xFFFFFF; st.bp = 0; st.ber = 0;
    for (int i = 0; i < 3; i++) { st.low = (int)((unsigned)st.low << 8) + bytes[st.bp]; st.bp++; }
    int maxlag = 8; if (d->dms == 25) maxlag /= 2; if (d->dms == 50) maxlag /= 2;
    int ber_why = 0;
    for (int n = 0; n < nfilt; n++) if (tns_order[n] > 0) {
        tns_order[n] = ad_decode(&st, &lc3t_tns_order_cum[s->lpc_weighting * 9], 8) + 1;
        if (st.ber) LC3O_BER(LC3O_REJ_TNS_SYMBOL);
        if (tns_order[n] > maxlag) { st.ber = 1; LC3O_BER(LC3O_REJ_TNS_ORDER); }
        for (int k = 0; k < tns_order[n]; k++) {
            if (r->bp < st.bp) { LC3O_REJECT(LC3O_REJ_TNS_READER); return 1; }
            tns_idx[n * 8 + k] = ad_decode(&st, &lc3t_tns_coef_cum[k * 18], 17);
            if (st.ber) LC3O_BER(LC3O_REJ_TNS_SYMBOL);
        }
    }
    if (st.ber > 0) { LC3O_REJECT(ber_why); return 1; }
    int c = 0, save_lev[LC3O_MAX_N];
    memset(save_lev, 0, sizeof save_lev);
    for (int k = 0; k < lastnz; k += 2) {
        int t = c + rate;
        if (k > L / 2) t += 256;
        x[k] = 0; x[k + 1] = 0;
        const int max_lev = d->hrmode == 1 ? 13 + 8 : 13;
        int lev, sym = 0;
        for (lev = 0; lev <= max_lev; lev++) {
            const int pki = lc3t_ac_ctx_lut[t + IMIN(lev, 3) * 1024];
            sym = ad_decode(&st, &lc3t_ac_cum[pki * 18], 17);
            if (st.ber) LC3O_BER(LC3O_REJ_SPEC_SYMBOL);
            if (sym < 16) break;
            if (lsbMode == 0 || lev > 0) { x[k] += rd_bit(r) << lev; x[k + 1] += rd_bit(r) << lev; }
        }
        if ((lev - 1) == 13 && sym == 16) { st.ber = 1; LC3O_BER(LC3O_REJ_ESCAPE_14); }
        if (d->hrmode == 0) lev = IMIN(lev, 13);
        if (lsbMode == 1) save_lev[k] = lev;
        const int a = sym & 3, b = sym >> 2;
        x[k] += a << lev; x[k + 1] += b << lev;
        if (x[k] > 0 && rd_bit(r) == 1) x[k] = -x[k];
        if (x[k + 1] > 0 && rd_bit(r) == 1) x[k + 1] = -x[k + 1];
        const int lev1 = IMIN(lev, 3);
        t = lev1 <= 1 ? 1 + (a + b) * (lev1 + 1) : 12 + lev1;
        c = (c & 15) * 16 + t;
        if (st.bp - r->bp > 3) { LC3O_REJECT(LC3O_REJ_OVERLAP); return 1; }
        if (st.ber > 0) { LC3O_REJECT(ber_why); return 1; }
    }
    const int nbits_side = total_bits - (8 * (r->bp + 1) + 8 - flog2_of(r->mask));
    const int nbits_ari = (st.bp + 1 - 3) * 8 + 25 - flog2_of((int)st.range);      /* floor(log2f(.)) with glibc's float log2 in both oracle builds, as in the encoder */
    *nres = total_bits - (nbits_side + nbits_ari);
    if (*nres < 0) { LC3O_REJECT(LC3O_REJ_NRES); return 1; }
    *res_present = 0;
    if (lsbMode == 0) {
        int nnz = 0;
        for (int k = 0; k < L; k++) nnz += x[k] != 0;
        if (d->hrmode) nnz *= 20;
        *nres = IMIN(*nres, nnz);
        *res_present = 1;
        memset(resBits, 0, LC3O_RESB);
        for (int k = 0; k < *nres; k++) resBits[k >> 3] |= rd_bit(r) << (k & 7);
    } else {
        for (int k = 0; k < lastnz; k += 2) if (save_lev[k] > 0) {
            for (int q = 0; q < 2; q++) {
                if (*nres == 0) goto lsb_done;
                int bit = rd_bit(r); (*nres)--;
                if (bit == 1) {
                    if (x[k + q] > 0) x[k + q]++;
                    else if (x[k + q] < 0) x[k + q]--;
                    else {
                        if (*nres == 0) goto lsb_done;
                        bit = rd_bit(r); (*nres)--;
                        x[k + q] = bit == 0 ? 1 : -1;
                    }
                }
            }
        }
        lsb_done:;
    }
    {   /* noise-filling seed R/ari_codec.c:31-45 */
        int sd = 0;
        for (int k = 0; k < L; k++) sd += abs(x[k]) * k;
        sd &= 65535; if (sd >= 32768) sd -= 65536;
        *nf_seed = sd;
    }
    *zero_frame = (lastnz == 2 && x[0] == 0 && x[1] == 0 && gg == 0 && fac_ns == 7);
    return 0;
}

/* MPVQ de-indexing R/sns_quantize_scf.c:432-480 */
static void dec_pvq(int k, int m, int ls_ind, int ind, int* pulses)
{
    int sign = 1 - 2 * ls_ind;
    for (int pos = 0; pos < m; pos++) {
        int k_delta;
        if (ind != 0) {
            const uint32_t* A = &lc3t_mpvq_offs[(m - pos - 1) * 11];
            int idx = 0;
            for (int i = 0; i < k + 1; i++) if ((uint32_t)ind >= A[i]) idx++;
            if (idx > 0) idx--;
            ind -= (int)A[idx];
            k_delta = k - idx;
        } else { pulses[pos] = sign * k; break; }
        if (k_delta != 0) {
            pulses[pos] = sign * k_delta;
            sign = (ind % 2) != 0 ? -1 : 1;
            ind = ind / 2;
            k -= k_delta;
        }
    }
}

/* R/sns_quantize_scf.c:482-544 */
static void dec_sns(const lc3o_dec* d, const int* scf_idx, float* scf_q)
{
    int pulses[16] = {0}, pulses2[6] = {0};
    for (int i = 0; i < 8; i++) { scf_q[i] = lc3t_sns_lf[scf_idx[0] * 8 + i]; scf_q[i + 8] = lc3t_sns_hf[scf_idx[1] * 8 + i]; }
    const int submode = scf_idx[2];
    if (submode < 2) {
        dec_pvq(10, 10, scf_idx[4], scf_idx[5], pulses);
        if (submode == 0) { dec_pvq(1, 6, scf_idx[6] % 2, scf_idx[6] / 2, pulses2); memcpy(&pulses[10], pulses2, sizeof pulses2); }
        else pulses[15] = 0;
    } else if (submode == 2) dec_pvq(8, 16, scf_idx[4], scf_idx[5], pulses);
    else dec_pvq(6, 16, scf_idx[4], scf_idx[5], pulses);
    float sum = 0, v[16], vi[16];
    for (int i = 0; i < 16; i++) sum += pulses[i] * pulses[i];
    sum = sqrtf(sum);
    for (int i = 0; i < 16; i++) v[i] = pulses[i] / sum;
    {   /* idct_II R/sns_quantize_scf.c:19-41 */
        const float n1 = sqrtf(2.0 / (float)16), n2 = 1.0 / (sqrtf(2.0));
        for (int i = 0; i < 16; i++) {
            float acc = 0;
            for (int j = 0; j < 16; j++) { float t = v[j] * d->idct_cos[i][j]; if (j == 0) t *= n2; acc += t; }
            vi[i] = n1 * acc;
        }
    }
    for (int i = 0; i < 16; i++) vi[i] = vi[i] * lc3t_sns_dec_gains[submode * 8 + scf_idx[3]];
    for (int i = 0; i < 16; i++) scf_q[i] = scf_q[i] + vi[i];
}

/* R/sns_interpolate_scf.c:13-89 with encoder_side = 0, then R/mdct_shaping.c:13-22 */
static void dec_sns_shape(const lc3o_dec* d, const float* g, float* x)
{
    float gi[80] = {0}, tmp[80] = {0};
    gi[0] = g[0]; gi[1] = g[0];
    for (int n = 0; n <= 14; n++) {
        gi[n * 4 + 2] = g[n] + (g[n + 1] - g[n]) / 8.0;
        gi[n * 4 + 3] = g[n] + 3.0 * (g[n + 1] - g[n]) / 8.0;
        gi[n * 4 + 4] = g[n] + 5.0 * (g[n + 1] - g[n]) / 8.0;
        gi[n * 4 + 5] = g[n] + 7.0 * (g[n + 1] - g[n]) / 8.0;
    }
    gi[62] = g[15] + (g[15] - g[14]) / 8.0;
    gi[63] = g[15] + 3.0 * (g[15] - g[14]) / 8.0;
    const int nb = d->nbands;
    if (nb < 64) {
        const int dd = 64 - nb;
        if (dd < 32) {
            for (int n = 0, i = 0; n < 2 * dd; n += 2, i++) tmp[i] = (gi[n] + gi[n + 1]) / 2.0;
            for (int n = 1; n < dd; n++) gi[n] = gi[2 * n];
            for (int n = 2 * dd; n < 64; n++) gi[n - dd] = gi[n];
            memcpy(gi, tmp, sizeof(float) * dd);
        } else {
            const float ratio = fabsf((float)(1.0 - 32.0 / (float)nb));
            const int n4 = round(ratio * nb);
            for (int i = 0; i < n4; i++) tmp[i] = (gi[4 * i] + gi[4 * i + 1] + gi[4 * i + 2] + gi[4 * i + 3]) / 4.0;
            for (int i = 0; i < nb - n4; i++) tmp[n4 + i] = (gi[4 * n4 + 2 * i] + gi[4 * n4 + 2 * i + 1]) / 2.0;
            memcpy(gi, tmp, sizeof(float) * nb);
        }
    }
    for (int n = 0; n < nb; n++) gi[n] = m_powf(2, gi[n]);
    for (int b = 0; b < nb; b++) for (int j = d->bands[b]; j < d->bands[b + 1]; j++) x[j] = x[j] * gi[b];
}

/* R/imdct.c:13-59 (dct4_apply R/dct4.c:75-95) */
static void dec_imdct(const lc3o_dec* d, dchan_t* s, const float* y, float* x)
{
    const int N = d->N, h = N / 2, la = d->la, winLen = 2 * N;
    float tda[LC3O_MAX_N], ov[2 * LC3O_MAX_N], z[LC3O_MAX_N], scratch[2 * LC3O_MAX_N];
    for (int i = 0; i < h; i++) { cpx a = {y[2 * i], y[N - 2 * i - 1]}; cpx c = cmul_f(a, d->tw1[i]); z[2 * i] = c.r; z[2 * i + 1] = c.i; }
    if (!dft_any(z, h, scratch)) assert(!"unsupported transform length");
    for (int i = 0; i < h; i++) { cpx a = {z[2 * i], z[2 * i + 1]}; cpx t = cmul_f(a, d->tw2[i]); tda[2 * i] = t.r * d->dct4_norm; tda[N - 2 * i - 1] = -t.i * d->dct4_norm; }
    memcpy(ov, &tda[h], sizeof(float) * h);
    for (int i = 0; i < h; i++) ov[h + i] = -tda[N - 1 - i];
    for (int i = 0; i < h; i++) ov[N + i] = -tda[h - 1 - i];
    for (int i = 0; i < h; i++) ov[N + h + i] = -tda[i];
    for (int i = 0; i < winLen; i++) ov[i] = ov[i] * d->win[winLen - 1 - i];
    for (int i = la, j = 0; i < N; i++, j++) ov[i] = ov[i] + s->imdct_mem[j];
    memcpy(x, &ov[la], sizeof(float) * N);
    memcpy(s->imdct_mem, &ov[N + la], sizeof(float) * (winLen - (N + la)));
}

/* R/ltpf_decoder.c:13-316 */
static void dec_ltpf(const lc3o_dec* d, dchan_t* s, float* x, int bfi, int* param)
{
    const int fs = d->fs, N = d->N;
    int pitch_int = 0, pitch_fr = 0, p1 = 0, p2 = 0;
    float gain = 0, a1[12] = {0}, a2[12] = {0}, b1[12] = {0}, b2[12] = {0};
    const float conf_alpha = 0.85;
    if (bfi == 1) { param[0] = 0; param[1] = 0; }              /* concealMethod is always 0 in this build */
    if (bfi != 1) {
        if (param[0] == 1) {
            if (param[2] < (127 - 32) * 4) { pitch_int = 32 + param[2] / 4; pitch_fr = param[2] - ((pitch_int - 32) * 4); }
            else if (param[2] < ((127 - 32) * 4) + ((157 - 127) * 2)) {
                param[2] = param[2] - ((127 - 32) * 4);
                pitch_int = 127 + param[2] / 2; pitch_fr = param[2] - ((pitch_int - 127) * 2); pitch_fr = pitch_fr * 2;
            } else { pitch_int = param[2] + (157 - ((127 - 32) * 4) - ((157 - 127) * 2)); pitch_fr = 0; }
            float pitch = ((float)pitch_int + (float)pitch_fr / 4.0) * (float)fs / 12800.0;
            pitch = round(pitch * 4.0) / 4.0;
            pitch_int = floor(pitch);
            pitch_fr = (int)((pitch - (float)pitch_int) * 4.0);
        }
        if (s->ltpf_beta_idx < 0) param[1] = 0;
        gain = param[1] == 1 ? s->ltpf_beta : 0;
    }
    if (s->ltpf_beta > 0) {
        const int cls = (fs == 8000 || fs == 16000) ? 0 : fs == 24000 ? 1 : fs == 32000 ? 2 : 3;
        static const int ilr[4] = {4, 6, 8, 12};
        const int inter_len_r = ilr[cls], tilt_len = inter_len_r - 2, tilt_len_r = inter_len_r - 1;
        const int inter_len = IMAX(fs, 16000) / 8000;
        const int old_x_len = tilt_len, old_y_len = (228 * fs / 12800) + inter_len, Lx = old_x_len, Ly = old_y_len;
        static float buf_x[4 * LC3O_MAX_N], buf_y[4 * LC3O_MAX_N], buf_z[4 * LC3O_MAX_N];
        memset(buf_x, 0, sizeof buf_x); memset(buf_y, 0, sizeof buf_y);
        memcpy(buf_x, s->ltpf_mem_x, sizeof(float) * old_x_len); memcpy(&buf_x[old_x_len], x, sizeof(float) * N);
        memcpy(buf_y, s->ltpf_mem_y, sizeof(float) * old_y_len);
        const int N4 = fs * 0.0025, N34 = N - N4;
        const float* ifl = &lc3t_ltpf_dec_inter[cls * 48]; const float* tfl = &lc3t_ltpf_dec_tilt[cls * 48];
        if (s->ltpf_param_mem[1] == 1) {
            for (int i = 0; i < inter_len_r; i++) a1[i] = s->ltpf_mem_gain * ifl[s->ltpf_mem_pitch_fr * 12 + i];
            for (int i = 0; i < tilt_len_r; i++) b1[i] = conf_alpha * s->ltpf_mem_gain * tfl[s->ltpf_mem_beta_idx * 12 + i];
            p1 = s->ltpf_mem_pitch_int;
        }
        if (param[1] == 1) {
            for (int i = 0; i < tilt_len_r; i++) b2[i] = conf_alpha * gain * tfl[s->ltpf_beta_idx * 12 + i];
            for (int i = 0; i < inter_len_r; i++) a2[i] = gain * ifl[pitch_fr * 12 + i];
            p2 = pitch_int;
        }
#define LTPF_SUMS(bx, B, A, P, n0) float sum1 = 0, sum2 = 0; { int j = 0; for (int i = (n0); i >= (n0) - tilt_len; i--) { sum1 += (B)[j] * (bx)[i]; j++; } \
            j = 0; for (int i = Ly + (n0) - Lx - (P) + inter_len - 1; i >= Ly + (n0) - Lx - (P) - inter_len; i--) { sum2 += (A)[j] * buf_y[i]; j++; } }
        const int m1 = s->ltpf_param_mem[1];
        if (m1 == 0 && param[1] == 0) memmove(&buf_y[Ly], &buf_x[Lx], sizeof(float) * N4);
        else if (m1 == 1 && param[1] == 0) {
            for (int n = 0; n < N4; n++) { LTPF_SUMS(buf_x, b1, a1, p1, Lx + n)
                buf_y[Ly + n] = buf_x[Lx + n] - (((float)N4 - (float)n) / (float)N4) * sum1 + (((float)N4 - (float)n) / (float)N4) * sum2; }
        } else if (m1 == 0 && param[1] == 1) {
            for (int n = 0; n < N4; n++) { LTPF_SUMS(buf_x, b2, a2, p2, Lx + n)
                buf_y[Ly + n] = buf_x[Lx + n] - ((float)n / (float)N4) * sum1 + ((float)n / (float)N4) * sum2; }
        } else if (s->ltpf_mem_pitch_int == pitch_int && s->ltpf_mem_pitch_fr == pitch_fr) {
            for (int n = 0; n < N4; n++) { LTPF_SUMS(buf_x, b2, a2, p2, Lx + n)
                buf_y[Ly + n] = buf_x[Lx + n] - sum1 + sum2; }
        } else {
            for (int n = 0; n < N4; n++) { LTPF_SUMS(buf_x, b1, a1, p1, Lx + n)
                buf_y[Ly + n] = buf_x[Lx + n] - (((float)N4 - (float)n) / (float)N4) * sum1 + (((float)N4 - (float)n) / (float)N4) * sum2; }
            memmove(buf_z, buf_y, sizeof buf_z);
            for (int n = 0; n < N4; n++) {
                float sum1 = 0, sum2 = 0; int j = 0;
                for (int i = Ly + n; i >= Ly + n - tilt_len; i--) { sum1 += b2[j] * buf_z[i]; j++; }
                j = 0;
                for (int i = Ly + n - p2 + inter_len - 1; i >= Ly + n - p2 - inter_len; i--) { sum2 += a2[j] * buf_y[i]; j++; }
                buf_y[Ly + n] = buf_z[Ly + n] - ((float)n / (float)N4) * sum1 + ((float)n / (float)N4) * sum2;
            }
        }
        if (param[1] == 0) memmove(&buf_y[Ly + N4], &buf_x[Lx + N4], sizeof(float) * N34);
        else for (int n = 0; n < N34; n++) { LTPF_SUMS(buf_x, b2, a2, p2, Lx + N4 + n)
            buf_y[Ly + N4 + n] = buf_x[Lx + N4 + n] - sum1 + sum2; }
#undef LTPF_SUMS
        memcpy(x, &buf_y[Ly], sizeof(float) * N);
        memcpy(s->ltpf_mem_x, &buf_x[N], sizeof(float) * old_x_len);
        memcpy(s->ltpf_mem_y, &buf_y[N], sizeof(float) * old_y_len);
    }
    memcpy(s->ltpf_param_mem, param, sizeof(int) * 3);
    s->ltpf_mem_pitch_int = pitch_int; s->ltpf_mem_pitch_fr = pitch_fr; s->ltpf_mem_gain = gain; s->ltpf_mem_beta_idx = s->ltpf_beta_idx;
}

/* one channel: R/dec_lc3_fl.c:13-130 */
static int dec_channel(lc3o_dec* d, dchan_t* s, const uint8_t* bs, void* out, int bps, int bfi)
{
    lc3o_dec_trace* tr = d->trace ? &d->trace[s - d->ch] : NULL;
    if (tr) memset(tr, 0, sizeof *tr);
    const int L = d->ylen, N = d->N;
    int gg = 0, fac_ns = 0, nfilt = 0, bw = 0, lastnz = 0, lsb = 0, nf_seed = 0, zero_frame = 0, res_present = 0, nres = 0;
    int tns_order[2] = {0, 0}, tns_idx[16] = {0}, scf_idx[7] = {0}, ltpf[3] = {0, 0, 0};
    static int xq[LC3O_MAX_N]; static uint8_t resBits[LC3O_RESB];
    float q[LC3O_MAX_N], xo[LC3O_MAX_N], scf_q[16];
    memset(q, 0, sizeof q);
    bitr r;
    s->last_reject = 0;
    if (bfi != 1) bfi = dec_side(d, bs, s->targetBytes, &r, &gg, scf_idx, &fac_ns, &nfilt, tns_order, ltpf, &bw, &lastnz, &lsb, &s->last_reject) ? 1 : bfi;
    if (bfi != 1) {
        memset(xq, 0, sizeof xq);
        if (dec_spectrum(d, s, bs, &r, nfilt, lsb, lastnz, tns_order, fac_ns, gg, resBits, xq, &nf_seed, tns_idx, &zero_frame, &nres, &res_present, &s->last_reject)) bfi = 1;
        for (int i = 0; i < L; i++) q[i] = (float)xq[i];
        if (tr) { tr->bw_idx = bw; tr->lastnz = lastnz; tr->lsb_mode = lsb; tr->gg_idx = gg; tr->fac_ns = fac_ns; tr->nfilt = nfilt; tr->nf_seed = nf_seed;
                  tr->zero_frame = zero_frame; tr->nres = nres; memcpy(tr->tns_order, tns_order, sizeof tns_order); memcpy(tr->tns_idx, tns_idx, sizeof tns_idx);
                  memcpy(tr->scf_idx, scf_idx, sizeof scf_idx); memcpy(tr->ltpf, ltpf, sizeof ltpf); memcpy(tr->xq, xq, sizeof(int) * L); }
    }
    if (bfi != 1) {
        dec_sns(d, scf_idx, scf_q);
        if (res_present) {                                         /* R/residual_decoding.c:13-96 */
            if (d->hrmode) {
                int nz[LC3O_MAX_N], nnz = 0, n = 0, iter = 0; float offset = 0.25;
                for (int k = 0; k < L; k++) if (q[k]) nz[nnz++] = k;
                while (n < nres && iter < 20) {
                    for (int k = 0; k < nnz; k++) {
                        if ((resBits[n >> 3] & 1 << (n & 7)) == 0) q[nz[k]] -= offset; else q[nz[k]] += offset;
                        if (++n >= nres) break;
                    }
                    offset /= 2; iter++;
                }
            } else {
                int k = 0, n = 0;
                while (k < L && n < nres) {
                    if (q[k] != 0) {
                        if ((resBits[n >> 3] & 1 << (n & 7)) == 0) { if (q[k] > 0) q[k] -= 0.1875f; else q[k] -= 0.3125f; }
                        else { if (q[k] > 0) q[k] += 0.3125f; else q[k] += 0.1875f; }
                        n++;
                    }
                    k++;
                }
            }
        }
        if (zero_frame == 0) {                                     /* R/noise_filling.c:13-80 */
            const int bw_stop = d->cut_bins[bw];
            const int tw = d->dms == 100 ? 3 : 1, so = d->dms == 100 ? 24 : d->dms == 50 ? 12 : 6;
            const float fac = (8.0 - fac_ns) / 16.0;
            int zl[LC3O_MAX_N], nz = 0;
            for (int k = so; k < bw_stop; k++) {
                int allz = 1;
                for (int i = k - tw; i <= IMIN(bw_stop - 1, k + tw); i++) if (q[i] != 0) allz = 0;
                if (allz) zl[nz++] = k;
            }
            for (int k = 0; k < nz; k++) {
                nf_seed = (13849 + (nf_seed + 32768) * 31821) & 65535;
                nf_seed -= 32768;
                q[zl[k]] = nf_seed >= 0 ? fac : -fac;
            }
        }
        {   /* R/apply_global_gain.c */
            const float g = m_powf(10, (float)(gg + s->gg_off) / 28);
            for (int i = 0; i < L; i++) q[i] = q[i] * g;
            if (tr) { memcpy(tr->q_gain, q, sizeof(float) * L); memcpy(tr->scf_q, scf_q, sizeof scf_q); }
        }
        {   /* R/tns_decoder.c:13-51 */
            const int bwb = d->cut_bins[bw];
            int start[2], stop[2]; float rc[9] = {0}, st[9] = {0};
            start[0] = (600 * s->N_red_tns * 2 / s->fs_red_tns) + 1;
            if (nfilt == 2) { stop[0] = bwb / 2; start[1] = bwb / 2 + 1; stop[1] = bwb; } else { stop[0] = bwb; start[1] = stop[1] = 0; }
            for (int f = 0; f < nfilt; f++) if (tns_order[f] > 0) {
                for (int j = 0; j < 8; j++) rc[j] = lc3t_tns_rc_pts[tns_idx[f * 8 + j]];
                const int ord = tns_order[f];
                for (int m = start[f]; m <= stop[f]; m++) {
                    float sv = q[m - 1] - rc[ord - 1] * st[ord - 1];
                    for (int l = ord - 2; l >= 0; l--) { sv = sv - rc[l] * st[l]; st[l + 1] = rc[l] * sv + st[l]; }
                    st[0] = sv; q[m - 1] = sv;
                }
            }
        }
        if (tr) memcpy(tr->q_tns, q, sizeof(float) * L);
        dec_sns_shape(d, scf_q, q);
    }
    /* PLC: R/plc_main.c:13-53, R/plc_noise_substitution0.c:13-46 */
    if (bfi == 1) {
        s->nbLost++;
        const float alpha = s->nbLost < 4 ? 1.0 : s->nbLost < 8 ? 0.9 : 0.85;
        s->cum_alpha = s->cum_alpha * alpha;
        for (int i = 0; i < L; i++) {
            s->plc_seed = 16831 + s->plc_seed * 12821;
            s->plc_seed = s->plc_seed - round((float)(s->plc_seed) * m_powf(2, -16)) * m_powf(2, 16);
            if (s->plc_seed == 32768) s->plc_seed -= 32768;
            q[i] = s->plc_seed < 0 ? s->q_d_prev[i] * (-s->cum_alpha) : s->q_d_prev[i] * s->cum_alpha;
        }
    } else memcpy(s->q_d_prev, q, sizeof(float) * L);
    if (tr) { tr->bfi = bfi; memcpy(tr->q_shaped, q, sizeof(float) * L); }
    dec_imdct(d, s, q, xo);
    if (tr) memcpy(tr->x_imdct, xo, sizeof(float) * N);
    if (bfi != 1) { s->nbLost = 0; s->cum_alpha = 1; }              /* R/plc_update.c:13-30 */
    s->prevprevBfi = s->prevBfi; s->prevBfi = bfi;
    dec_ltpf(d, s, xo, bfi, ltpf);
    if (tr) memcpy(tr->x_out, xo, sizeof(float) * N);
    if (bps == 16) {
        for (int i = 0; i < N; i++) { const float t = round(m_powf(2, 16 - 1) * (xo[i] * m_powf(2, -15))); ((int16_t*)out)[i] = (int16_t)fmaxf(fminf(t, 32767), -32768); }
    } else {
        for (int i = 0; i < N; i++) ((int32_t*)out)[i] = (int32_t)round(m_powf(2, bps - 1) * (xo[i] * m_powf(2, -15)));
    }
    return bfi;
}

/* R/dec_lc3_fl.c:133-161 + R/lc3.c:277-282.  Returns 0, LC3O_DECODE_ERROR (frame concealed) or a configuration error. */
int lc3o_dec_frame(lc3o_dec* d, const uint8_t* input, int num_bytes, void** output, int bps, int bfi_ext)
{
    if (!d || !input || !output) return LC3O_NULL_ERROR;
    if (!d->win) return LC3O_UNSUPPORTED;
    int bfi = bfi_ext;
    if (bfi == 0) bfi = !num_bytes;
    for (int ch = 0; ch < d->channels; ch++) {
        dchan_t* s = &d->ch[ch];
        const int nb2 = num_bytes / d->channels + (ch < (num_bytes % d->channels));
        if (bfi != 1 && nb2 != s->last_size) {
            const int err = dec_bitrate(d, s, nb2);
            if (err) return err;
            s->last_size = nb2;
        }
        bfi = dec_channel(d, s, input, output[ch], bps, bfi);
        input += s->targetBytes;
    }
    return bfi == 1 ? LC3O_DECODE_ERROR : 0;
}
#undef LC3O_REJECT
#undef LC3O_BER
