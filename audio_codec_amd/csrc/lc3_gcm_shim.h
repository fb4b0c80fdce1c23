/* lc3_gcm_shim.h -- Secure RTP with the AEAD suites of RFC 7714, AEAD_AES_128_GCM and AEAD_AES_256_GCM (include/lc3plus_batch.h "Secure RTP, AEAD":
 * lc3plus_srtp_gcm_make_context, lc3plus_{enc,dec}_batch_srtp_gcm_protect, lc3plus_dec_batch_srtp_gcm_unprotect, lc3plus_plan_srtp_gcm_protect,
 * lc3plus_plan_srtp_gcm_unprotect): what the host C code (lc3_packet.c) and the sibling library that holds the kernels (lc3_gcm.hip -> liblc3plus_gcm_hip.so)
 * share.  Everything around the transform is lc3_srtp_shim.h's as it stands: the AES table, the fetch, align and sink helpers, the receive checks (lc3s_check
 * with a tag of 16 bytes), the index estimate, the window and state functions, the rollover counter of a sent packet, the workspace and the two call structs.
 * This file adds the key expansion for 16- and 32-byte keys, the AES block with the round count as an argument, GHASH, the GCM walk over a packet's words and
 * the two rules, one text for the host functions and the kernels.  The lc3gcm_* functions are the sibling's whole C ABI.  lc3_packet.c loads the sibling from
 * its own directory on the first GCM call; the seven other code objects hold none of this. */
#ifndef LC3_GCM_SHIM_H
#define LC3_GCM_SHIM_H
#include "lc3_srtp_shim.h"

/* LC3PLUS_SRTP_GCM_* of include/lc3plus_batch.h: the words of a context - round keys (44 or 60 of the 60), the number of rounds, the session salt, the GHASH
 * table - and the tag's length */
enum { LC3G_CTX_WORDS = 128, LC3G_CTX_RK = 0, LC3G_CTX_ROUNDS = 60, LC3G_CTX_SALT = 61, LC3G_CTX_TABLE = 64, LC3G_TAG_BYTES = 16 };
/* what a walk does with the words it passes: hash them (header and ciphertext), XOR the payload's with the keystream, hand them to the sink */
enum { LC3G_HASH = 1, LC3G_CRYPT = 2, LC3G_STORE = 4 };
/* Where the kernels read the GHASH table: 1, from a copy in LDS that every lane makes before its walk, lane-interleaved (the product: the faster by a third in
 * the comparison of DESIGN 10l); 0, from the context in global memory, 16 bytes per step (a build with -DLC3G_LDS_TABLE=0 for that comparison) */
#ifndef LC3G_LDS_TABLE
#define LC3G_LDS_TABLE 1
#endif

/* ---- AES with 10 or 14 rounds ---- */
/* FIPS-197 5.2 for Nk = 4 or 8: the 4 * (rounds + 1) round key words of a 16- or 32-byte key, every word big-endian */
static inline LC3S_HD void lc3g_expand(const uint32_t* te, const uint8_t* key, int key_bytes, uint32_t rk[60])
{
    const int nk = key_bytes / 4, n = 4 * (nk + 7);
    for (int i = 0; i < nk; i++) rk[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 | (uint32_t)key[4 * i + 2] << 8 | key[4 * i + 3];
    uint32_t rc = 1;
    for (int i = nk; i < n; i++) {
        uint32_t t = rk[i - 1];
        if (i % nk == 0) t = lc3s_rotl(t, 8);
        if (i % nk == 0 || (nk == 8 && i % nk == 4))
            t = lc3s_sbox(te, t >> 24) << 24 | lc3s_sbox(te, (t >> 16) & 255u) << 16 | lc3s_sbox(te, (t >> 8) & 255u) << 8 | lc3s_sbox(te, t & 255u);
        if (i % nk == 0) { t ^= rc << 24; rc = lc3s_xtime(rc); }
        rk[i] = rk[i - nk] ^ t;
    }
}
/* FIPS-197 5.1 on big-endian column words, lc3s_aes with the number of rounds nr (10 or 14) an argument: (i0 .. i3) -> (*o0 .. *o3) */
static inline LC3S_HD LC3S_INL void lc3g_aes(const uint32_t* te, int nt, const uint32_t* rk, int nr, uint32_t i0, uint32_t i1, uint32_t i2, uint32_t i3, uint32_t* o0,
                                             uint32_t* o1, uint32_t* o2, uint32_t* o3)
{
    uint32_t s0 = i0 ^ rk[0], s1 = i1 ^ rk[1], s2 = i2 ^ rk[2], s3 = i3 ^ rk[3];
    for (int r = 1; r < nr; r++) {
        const uint32_t* k = rk + 4 * r;
        const uint32_t t0 = lc3s_te(te, nt, 0, s0 >> 24) ^ lc3s_te(te, nt, 1, (s1 >> 16) & 255u) ^ lc3s_te(te, nt, 2, (s2 >> 8) & 255u) ^ lc3s_te(te, nt, 3, s3 & 255u) ^ k[0];
        const uint32_t t1 = lc3s_te(te, nt, 0, s1 >> 24) ^ lc3s_te(te, nt, 1, (s2 >> 16) & 255u) ^ lc3s_te(te, nt, 2, (s3 >> 8) & 255u) ^ lc3s_te(te, nt, 3, s0 & 255u) ^ k[1];
        const uint32_t t2 = lc3s_te(te, nt, 0, s2 >> 24) ^ lc3s_te(te, nt, 1, (s3 >> 16) & 255u) ^ lc3s_te(te, nt, 2, (s0 >> 8) & 255u) ^ lc3s_te(te, nt, 3, s1 & 255u) ^ k[2];
        const uint32_t t3 = lc3s_te(te, nt, 0, s3 >> 24) ^ lc3s_te(te, nt, 1, (s0 >> 16) & 255u) ^ lc3s_te(te, nt, 2, (s1 >> 8) & 255u) ^ lc3s_te(te, nt, 3, s2 & 255u) ^ k[3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    const uint32_t* k = rk + 4 * nr;
    *o0 = (lc3s_sbox(te, s0 >> 24) << 24 | lc3s_sbox(te, (s1 >> 16) & 255u) << 16 | lc3s_sbox(te, (s2 >> 8) & 255u) << 8 | lc3s_sbox(te, s3 & 255u)) ^ k[0];
    *o1 = (lc3s_sbox(te, s1 >> 24) << 24 | lc3s_sbox(te, (s2 >> 16) & 255u) << 16 | lc3s_sbox(te, (s3 >> 8) & 255u) << 8 | lc3s_sbox(te, s0 & 255u)) ^ k[1];
    *o2 = (lc3s_sbox(te, s2 >> 24) << 24 | lc3s_sbox(te, (s3 >> 16) & 255u) << 16 | lc3s_sbox(te, (s0 >> 8) & 255u) << 8 | lc3s_sbox(te, s1 & 255u)) ^ k[2];
    *o3 = (lc3s_sbox(te, s3 >> 24) << 24 | lc3s_sbox(te, (s0 >> 16) & 255u) << 16 | lc3s_sbox(te, (s1 >> 8) & 255u) << 8 | lc3s_sbox(te, s2 & 255u)) ^ k[3];
}

/* ---- GHASH ---- */
/* A block of SP 800-38D is held as four big-endian words, z[0] its first four bytes: the coefficient of x^i is bit 31 - i % 32 of word i / 32, so that a
 * multiplication by x is a shift to the right by one bit with 1 + x + x^2 + x^7 (E1 in the top byte) folded in for the bit that falls out.
 * The table is M[e] = e(x) * H for the sixteen nibbles e, whose highest bit is the lowest power: M[8] = H, M[4] = H x, M[2] = H x^2, M[1] = H x^3 and the
 * rest their sums; four words each, 256 bytes.  `tab` is word 0 of entry 0 and `ts` the distance between two words of it in words: 1 in a context, the
 * workgroup's lanes where the kernels keep a lane-interleaved copy in LDS. */
static inline void lc3g_table(const uint32_t h[4], uint32_t tab[64])
{
    for (int i = 0; i < 64; i++) tab[i] = 0;
    uint32_t v[4] = {h[0], h[1], h[2], h[3]};
    for (int e = 8; e; e >>= 1) {
        for (int w = 0; w < 4; w++) tab[4 * e + w] = v[w];
        const uint32_t fold = (0u - (v[3] & 1u)) & 0xE1000000u;
        v[3] = v[3] >> 1 | v[2] << 31; v[2] = v[2] >> 1 | v[1] << 31; v[1] = v[1] >> 1 | v[0] << 31; v[0] = v[0] >> 1 ^ fold;
    }
    for (int e = 2; e < 16; e <<= 1)
        for (int j = 1; j < e; j++)
            for (int w = 0; w < 4; w++) tab[4 * (e + j) + w] = tab[4 * e + w] ^ tab[4 * j + w];
}
/* eight steps Z = Z x^4 + M[nibble] over the nibbles of the word xw, the last first.  The four bits r that fall out of Z come back as r(x) x^128, which is
 * the carry-less product of r and 1C20 in the top sixteen bits (RED[r] of the classic table; 1C20 has the bits 12, 11, 10 and 5) */
static inline LC3S_HD LC3S_INL void lc3g_mul_word(uint32_t z[4], uint32_t xw, const uint32_t* tab, int ts)
{
    for (int n = 0; n < 8; n++) {
        const uint32_t e = (xw >> (4 * n)) & 15u, r = z[3] & 15u;
        const uint32_t* m = tab + (size_t)(4 * e) * (size_t)ts;
        const uint32_t m0 = m[0], m1 = m[ts], m2 = m[2 * ts], m3 = m[3 * ts];
        z[3] = (z[3] >> 4 | z[2] << 28) ^ m3;
        z[2] = (z[2] >> 4 | z[1] << 28) ^ m2;
        z[1] = (z[1] >> 4 | z[0] << 28) ^ m1;
        z[0] = z[0] >> 4 ^ (r << 28 ^ r << 27 ^ r << 26 ^ r << 21) ^ m0;
    }
}
/* Z <- Z * H, Z holding the sum of the hash so far and the next block: 32 steps, from the block's last nibble to its first */
static inline LC3S_HD LC3S_INL void lc3g_mul(uint32_t z[4], const uint32_t* tab, int ts)
{
    const uint32_t x0 = z[0], x1 = z[1], x2 = z[2], x3 = z[3];
    z[0] = z[1] = z[2] = z[3] = 0;
    lc3g_mul_word(z, x3, tab, ts);
    lc3g_mul_word(z, x2, tab, ts);
    lc3g_mul_word(z, x1, tab, ts);
    lc3g_mul_word(z, x0, tab, ts);
}

/* ---- the walk over a packet ---- */
/* RFC 7714 8.1 and 9, SP 800-38D 7.1: a packet of L bytes at p whose payload begins at byte 4 * h4 (a header is a whole number of words).  The 12-byte IV is
 * (00 00 || SSRC || roc || SEQ) XOR the session salt; counter block IV || 1 masks the tag and the payload's block j is XORed with AES_k(IV || 2 + j).  The
 * words k0 .. of the packet are fetched as aligned words and realigned (lc3s_aw, lc3s_align), the bytes behind L zero, and by `mode`: the payload's are XORed
 * with the keystream (LC3G_CRYPT), every word is added into the hash at its place in its block, the header's and the payload's each padded with zeros to
 * whole blocks, the payload's after the XOR (LC3G_HASH: k0 is 0 then), and handed to the sink (LC3G_STORE).  With LC3G_HASH tag[0 .. 3] is
 * GHASH_H(header, payload) ^ AES_k(IV || 1) as four big-endian words: for a packet that is protected the tag itself, for a received one what its last 16 bytes
 * must equal, the walk being run without LC3G_CRYPT over the ciphertext.  A packet takes (4 * h4 + 15) / 16 + (L - 4 * h4 + 15) / 16 + 1 multiplications by H
 * and (L - 4 * h4 + 15) / 16 + 1 AES blocks. */
static inline LC3S_HD LC3S_INL void lc3g_walk(const uint32_t* ctx, const uint32_t* te, int nt, const uint32_t* tab, int ts, const uint8_t* p, int L, int h4, int k0, int mode,
                                              uint32_t ssrc, uint32_t roc, uint32_t seq, lc3s_sink* out, uint32_t tag[4])
{
    const uint32_t* rk = ctx + LC3G_CTX_RK;
    const int nr = (int)ctx[LC3G_CTX_ROUNDS];
    const uint32_t iv0 = ctx[LC3G_CTX_SALT] ^ ssrc >> 16, iv1 = ctx[LC3G_CTX_SALT + 1] ^ (ssrc << 16 | roc >> 16), iv2 = ctx[LC3G_CTX_SALT + 2] ^ (roc << 16 | seq);
    uint32_t sh, ks0 = 0, ks1 = 0, ks2 = 0, ks3 = 0;
    uint32_t z[4] = {0, 0, 0, 0};
    const uint8_t* base = lc3s_base(p, &sh);
    const int end = (int)sh + L;
    uint32_t cur = lc3s_aw(base, k0, end);
    for (int k = k0; 4 * k < L; k++) {
        const uint32_t nxt = lc3s_aw(base, k + 1, end);
        uint32_t m = lc3s_bswap(lc3s_align(nxt, cur, sh));
        cur = nxt;
        const uint32_t keep = 4 * k + 4 > L ? ~0u << (8 * (4 * k + 4 - L)) : ~0u;
        m &= keep;
        const uint32_t q = (uint32_t)(k >= h4 ? k - h4 : k) & 3u;
        if ((mode & LC3G_CRYPT) && k >= h4) {
            if (q == 0) lc3g_aes(te, nt, rk, nr, iv0, iv1, iv2, 2u + ((uint32_t)(k - h4) >> 2), &ks0, &ks1, &ks2, &ks3);
            m ^= (q == 0 ? ks0 : q == 1 ? ks1 : q == 2 ? ks2 : ks3) & keep;
        }
        if (mode & LC3G_STORE) lc3s_put(out, k, lc3s_bswap(m));
        if (mode & LC3G_HASH) {
            z[0] ^= q == 0 ? m : 0u; z[1] ^= q == 1 ? m : 0u; z[2] ^= q == 2 ? m : 0u; z[3] ^= q == 3 ? m : 0u;
            if (q == 3 || k == h4 - 1 || 4 * k + 4 >= L) lc3g_mul(z, tab, ts);
        }
    }
    if (mode & LC3G_STORE) lc3s_flush(out);
    if (mode & LC3G_HASH) {
        z[1] ^= (uint32_t)(4 * h4) * 8u; z[3] ^= (uint32_t)(L - 4 * h4) * 8u;       /* the lengths in bits, 64 bits each: a packet has at most 2^20 bytes */
        lc3g_mul(z, tab, ts);
        lc3g_aes(te, nt, rk, nr, iv0, iv1, iv2, 1u, &ks0, &ks1, &ks2, &ks3);
        tag[0] = z[0] ^ ks0; tag[1] = z[1] ^ ks1; tag[2] = z[2] ^ ks2; tag[3] = z[3] ^ ks3;
    }
}

/* ---- the context (host only) ---- */
/* RFC 7714 11: the key derivation of RFC 3711 4.3.1 (lc3s_derive) with key derivation rate 0, the 12-byte master salt followed by two zero bytes in the
 * 14-byte salt's place and AES-CM under the master key - AES-128 for 16 bytes, AES-256 (RFC 6188) for 32 - as the PRF.  te: Te0, 256 words; mrk, nr: the
 * master key's round keys and rounds */
static inline void lc3g_derive(const uint32_t* te, const uint32_t mrk[60], int nr, const uint8_t master_salt[12], int label, uint8_t* out, int n)
{
    uint8_t x[16];
    for (int i = 0; i < 12; i++) x[i] = master_salt[i];
    x[12] = x[13] = x[14] = x[15] = 0;
    x[7] ^= (uint8_t)label;
    uint32_t iv[4];
    for (int i = 0; i < 4; i++) iv[i] = (uint32_t)x[4 * i] << 24 | (uint32_t)x[4 * i + 1] << 16 | (uint32_t)x[4 * i + 2] << 8 | x[4 * i + 3];
    for (int j = 0; 16 * j < n; j++) {
        uint32_t o[4];
        lc3g_aes(te, 1, mrk, nr, iv[0], iv[1], iv[2], iv[3] + (uint32_t)j, &o[0], &o[1], &o[2], &o[3]);
        for (int b = 0; b < 16 && 16 * j + b < n; b++) out[16 * j + b] = (uint8_t)(o[b >> 2] >> (8 * (3 - (b & 3))));
        lc3s_wipe(o, sizeof o);
    }
}
/* key_bytes: 16 or 32.  Label 0 gives the session key (key_bytes bytes), label 2 the session salt (12 bytes); there is no authentication key.  H = AES_k(0).
 * The working copies are wiped as lc3s_make_context wipes its own */
static inline void lc3g_make_context(const uint8_t* master_key, int key_bytes, const uint8_t master_salt[12], int32_t ctx[LC3G_CTX_WORDS])
{
    uint32_t te[LC3S_TE_WORDS], mrk[60], c[LC3G_CTX_WORDS], h[4];
    uint8_t ke[32], ks[12];
    const int nr = key_bytes / 4 + 6;
    for (uint32_t x = 0; x < LC3S_TE_WORDS; x++) te[x] = lc3s_te0(x);
    lc3g_expand(te, master_key, key_bytes, mrk);
    lc3g_derive(te, mrk, nr, master_salt, 0, ke, key_bytes);
    lc3g_derive(te, mrk, nr, master_salt, 2, ks, 12);
    for (int i = 0; i < LC3G_CTX_WORDS; i++) c[i] = 0;
    lc3g_expand(te, ke, key_bytes, c + LC3G_CTX_RK);
    c[LC3G_CTX_ROUNDS] = (uint32_t)nr;
    for (int i = 0; i < 3; i++) c[LC3G_CTX_SALT + i] = (uint32_t)ks[4 * i] << 24 | (uint32_t)ks[4 * i + 1] << 16 | (uint32_t)ks[4 * i + 2] << 8 | ks[4 * i + 3];
    lc3g_aes(te, 1, c + LC3G_CTX_RK, nr, 0u, 0u, 0u, 0u, &h[0], &h[1], &h[2], &h[3]);
    lc3g_table(h, c + LC3G_CTX_TABLE);
    for (int i = 0; i < LC3G_CTX_WORDS; i++) ctx[i] = (int32_t)c[i];
    lc3s_wipe(mrk, sizeof mrk); lc3s_wipe(c, sizeof c); lc3s_wipe(h, sizeof h); lc3s_wipe(ke, sizeof ke); lc3s_wipe(ks, sizeof ks);
}

/* ---- the protect rule ---- */
/* lc3s_protect with the GCM walk in the HMAC's place: the statuses and their order, the packet's address and length, the rollover counter and the destination
 * are that function's, the tag's length is 16 (q->tag_len is not read) and a route's context has LC3G_CTX_WORDS words.  tab, ts: the route's GHASH table where
 * the caller keeps a copy, NULL for the context's own */
static inline LC3S_HD int lc3g_protect(const lc3s_protect_in* q, long long p, const uint32_t* te, int nt, const uint32_t* tab, int ts, int32_t* out_size)
{
    *out_size = 0;
    if (!(q->status[p] & LC3R_STAMPED)) return LC3S_NOT_STAMPED;
    const int r = q->route[p];
    if (r < 0 || r >= q->n_routes) return LC3S_BAD_ROUTE;
    const long long off = q->offset[p];
    const int32_t size = q->size[p];
    if (off < 0 || size < q->header_room || size > LC3S_MAX_PACKET || off > q->wire_capacity - size) return LC3S_PR_RANGE;      /* size >= 12: no overflow */
    const long long a = off + q->header_room - q->payload_room - LC3R_FIXED;
    const int L = size - q->header_room + q->payload_room + LC3R_FIXED;
    if ((long long)L + LC3G_TAG_BYTES > q->dst_stride || p >= q->dst_capacity / q->dst_stride) return LC3S_PR_OVERFLOW;
    uint32_t hw[3];
    lc3r_fetch12(q->wire, a, hw);
    const uint32_t seq = hw[0] & 0xFFFFu, ssrc = hw[2];
    const uint32_t roc = lc3s_roc_at((uint32_t)q->roc[r], (uint32_t)q->seq_base[r], seq);
    const uint32_t* ctx = (const uint32_t*)q->ctx + (size_t)r * LC3G_CTX_WORDS;
    uint8_t* d = q->dst + p * q->dst_stride;
    lc3s_sink out;
    uint32_t tag[4];
    lc3s_sink_init(&out, d, 0, L);
    lc3g_walk(ctx, te, nt, tab ? tab : ctx + LC3G_CTX_TABLE, tab ? ts : 1, q->wire + a, L, LC3R_FIXED / 4, 0, LC3G_HASH | LC3G_CRYPT | LC3G_STORE, ssrc, roc, seq, &out, tag);
    lc3s_sink_init(&out, d + L, 0, LC3G_TAG_BYTES);                   /* the tag behind the ciphertext, through a sink of its own: whole words where they are the tag's */
    for (int i = 0; i < 4; i++) lc3s_put(&out, i, lc3s_bswap(tag[i]));
    lc3s_flush(&out);
    *out_size = L + LC3G_TAG_BYTES;
    return LC3S_PROTECTED;
}

/* ---- the unprotect rule ---- */
/* lc3s_unprotect with the GCM walks in the HMAC's and the keystream's place.  Checks 3 and 4 restate that function's first lines, which it does not give apart
 * from its transform; lc3_srtp_shim.h stays as it is so that the SRTP code object does, and whoever changes one text changes the other
 * (tests/test_gcm_cpu.py holds both to one restatement of the window on the same scenarios).  Check 5 hashes the header and the ciphertext without storing,
 * compares all 16 bytes behind them, and only then decrypts [h, size - 16) in place */
static inline LC3S_HD int lc3g_unprotect(uint8_t* ring, long long off, int32_t size, const lc3s_item* it, const int32_t* state, uint32_t s_l_first, const uint32_t* ctx,
                                         const uint32_t* te, int nt, const uint32_t* tab, int ts, long long* index)
{
    const int started = state[LC3S_FLAGS] & LC3S_STARTED;
    const uint32_t sroc = (uint32_t)state[LC3S_ROC], s_l = started ? (uint32_t)state[LC3S_S_L] & 0xFFFFu : s_l_first;
    int refused;
    const uint32_t roc = lc3s_guess(sroc, s_l, (uint32_t)it->seq, &refused);
    *index = 0;
    if (refused) return LC3S_REPLAY_OLD;
    const long long idx = (long long)roc << 16 | (long long)it->seq;
    if (started) {
        const long long delta = ((long long)sroc << 16 | (long long)s_l) - idx;
        if (delta >= LC3S_WINDOW) return LC3S_REPLAY_OLD;
        if (delta >= 0) {
            const uint32_t half = (uint32_t)state[delta < 32 ? LC3S_WIN_LO : LC3S_WIN_HI];
            if ((half >> (delta & 31)) & 1u) return LC3S_REPLAYED;
        }
    }
    const int L = size - LC3G_TAG_BYTES;
    uint8_t* p = ring + off;
    if (!tab) { tab = ctx + LC3G_CTX_TABLE; ts = 1; }
    lc3s_sink out;
    uint32_t tag[4], tsh, diff = 0;
    lc3s_sink_init(&out, p, it->h, L);
    lc3g_walk(ctx, te, nt, tab, ts, p, L, it->h / 4, 0, LC3G_HASH, it->ssrc, roc, (uint32_t)it->seq, &out, tag);
    const uint8_t* tb = lc3s_base(p + L, &tsh);                       /* the 16 bytes behind the ciphertext, as aligned words */
    uint32_t cur = lc3s_aw(tb, 0, (int)tsh + LC3G_TAG_BYTES);
    for (int i = 0; i < 4; i++) {
        const uint32_t nxt = lc3s_aw(tb, i + 1, (int)tsh + LC3G_TAG_BYTES);
        diff |= lc3s_bswap(lc3s_align(nxt, cur, tsh)) ^ tag[i];
        cur = nxt;
    }
    if (diff) return LC3S_AUTH;
    lc3g_walk(ctx, te, nt, tab, ts, p, L, it->h / 4, it->h / 4, LC3G_CRYPT | LC3G_STORE, it->ssrc, roc, (uint32_t)it->seq, &out, tag);
    *index = idx;
    return LC3S_OK;
}

#ifdef __cplusplus
extern "C" {
#endif
/* queue the kernels on q->hip_stream; wait for them only with q->sync.  0, or 1 where nothing was queued.  The call structs are the SRTP library's; tag_len
 * is 16 in both */
int lc3gcm_protect_run(const lc3srtp_protect_call* q);
int lc3gcm_unprotect_run(const lc3srtp_unprotect_call* q);
/* launches of a GCM kernel by this process, by the kernel's symbol name in the code object; -1 for a name the library does not hold */
long long lc3gcm_launch_count(const char* kernel);
#ifdef __cplusplus
}
#endif
#endif
