/* lc3_srtp_shim.h -- Secure RTP (include/lc3plus_batch.h "Secure RTP": lc3plus_srtp_make_context, lc3plus_{enc,dec}_batch_srtp_protect,
 * lc3plus_dec_batch_srtp_unprotect, lc3plus_plan_srtp_protect, lc3plus_plan_srtp_unprotect): what the host C code (lc3_packet.c) and the sibling library that
 * holds the kernels (lc3_srtp.hip -> liblc3plus_srtp_hip.so) share.  AES-128 (key expansion, block encryption, the tables), the SHA-1 compression, the walk over
 * a packet's words that encrypts, hashes and stores, the protect rule, the receive checks, the index estimate and the window are one text for the host functions
 * and the kernels; they differ only in how a packet's bytes are fetched and stored (plain bytes on the host; aligned 32-bit words realigned in registers on the
 * device, whole-word stores where all four bytes are the packet's own).  The lc3srtp_* functions are the sibling's whole C ABI.  lc3_packet.c loads the sibling
 * from its own directory on the first SRTP call; the six other code objects hold none of this. */
#ifndef LC3_SRTP_SHIM_H
#define LC3_SRTP_SHIM_H
#include <stdint.h>
#include <stddef.h>
#include "lc3_rtp_shim.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LC3S_HD __host__ __device__
#define LC3S_UNROLL _Pragma("unroll")
/* functions that take a walk, a sink or a schedule by pointer: inlined whatever the optimiser weighs, so that those stay in registers */
#define LC3S_INL __attribute__((always_inline))
#else
#define LC3S_INL
#define LC3S_HD
#define LC3S_UNROLL
#endif

/* LC3PLUS_SRTP_* of include/lc3plus_batch.h: the words of a context and of a source's state, an item's status (also its word in stats), a packet's status */
enum { LC3S_CTX_WORDS = 64, LC3S_CTX_RK = 0, LC3S_CTX_SALT = 44, LC3S_CTX_IPAD = 48, LC3S_CTX_OPAD = 53, LC3S_CTX_USED = 58 };
enum { LC3S_STATE_WORDS = 8, LC3S_FLAGS = 0, LC3S_ROC = 1, LC3S_S_L = 2, LC3S_WIN_LO = 3, LC3S_WIN_HI = 4, LC3S_STARTED = 1, LC3S_WINDOW = 64 };
enum { LC3S_OK = 0, LC3S_RANGE = 1, LC3S_SHORT = 2, LC3S_VERSION = 3, LC3S_RTCP = 4, LC3S_HEADER = 5, LC3S_UNKNOWN_SSRC = 6, LC3S_REPLAY_OLD = 7, LC3S_REPLAYED = 8,
       LC3S_AUTH = 9, LC3S_STATUSES = 10, LC3S_STATS_WORDS = 16 };
enum { LC3S_PROTECTED = 1, LC3S_NOT_STAMPED = 2, LC3S_BAD_ROUTE = 4, LC3S_PR_RANGE = 8, LC3S_PR_OVERFLOW = 16 };
enum { LC3S_THREADS = 256, LC3S_TE_WORDS = 256 };
#define LC3S_MAX_ITEMS (1LL << 29)
#define LC3S_MAX_STRIDE (1LL << 30)
/* the longest packet or datagram either rule takes: the block counter is added into the IV's low 16 bits, which are zero, so a payload has at most 2^16 blocks */
#define LC3S_MAX_PACKET (1 << 20)
/* the AES tables the kernels keep in LDS: 1 (Te0, the others by rotation; the product) or 4 (Te0 .. Te3; a build with -DLC3S_NT=4 for the comparison of DESIGN 10k) */
#ifndef LC3S_NT
#define LC3S_NT 1
#endif

/* ---- AES-128 ---- */
static inline LC3S_HD uint32_t lc3s_rotl(uint32_t v, int n) { return v << n | v >> (32 - n); }
static inline LC3S_HD uint32_t lc3s_xtime(uint32_t a) { return ((a << 1) ^ ((a >> 7) * 0x1Bu)) & 255u; }
static inline LC3S_HD uint32_t lc3s_gmul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 0; i < 8; i++) { r ^= (0u - (b & 1u)) & a; a = lc3s_xtime(a); b >>= 1; }
    return r;
}
/* Entry x of the encryption table Te0: with s = S-box(x), the column (02 s, s, s, 03 s), its first byte highest.  The S-box is the inverse in GF(2^8), x^254,
 * under the affine map of FIPS-197 5.1.1; its byte is bits 8 .. 15 of the entry, so the one table serves the last round and the key expansion as well.  Te1, Te2
 * and Te3 are this entry rotated right by 8, 16 and 24 bits.  Nothing here is a table in the source: every workgroup and every host call computes its own */
static inline LC3S_HD uint32_t lc3s_te0(uint32_t x)
{
    uint32_t y = x, inv = 1;
    for (int i = 1; i < 8; i++) { y = lc3s_gmul(y, y); inv = lc3s_gmul(inv, y); }       /* y = x^(2^i); inv = x^(2 + 4 + ... + 128) */
    uint32_t s = inv | inv << 8;                                     /* the byte twice: a rotation of the byte is a shift of this */
    s = (s ^ s >> 4 ^ s >> 5 ^ s >> 6 ^ s >> 7 ^ 0x63u) & 255u;      /* inv ^ rotl(inv, 4) ^ rotl(inv, 3) ^ rotl(inv, 2) ^ rotl(inv, 1) ^ 63 */
    const uint32_t s2 = lc3s_xtime(s);
    return s2 << 24 | s << 16 | s << 8 | (s2 ^ s);
}
/* table k of `nt` tables at x: with four tables te holds Te0 .. Te3 one behind the other, with one it is Te0 and the others are rotations of it */
static inline LC3S_HD uint32_t lc3s_te(const uint32_t* te, int nt, int k, uint32_t x)
{
    if (nt == 4) return te[k * LC3S_TE_WORDS + x];
    const uint32_t v = te[x];
    return k ? v >> (8 * k) | v << (32 - 8 * k) : v;
}
static inline LC3S_HD uint32_t lc3s_sbox(const uint32_t* te, uint32_t x) { return (te[x] >> 8) & 255u; }
/* FIPS-197 5.2: the 44 round key words of a 16-byte key, every word big-endian */
static inline LC3S_HD void lc3s_expand(const uint32_t* te, const uint8_t key[16], uint32_t rk[44])
{
    for (int i = 0; i < 4; i++) rk[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 | (uint32_t)key[4 * i + 2] << 8 | key[4 * i + 3];
    uint32_t rc = 1;
    for (int i = 4; i < 44; i++) {
        uint32_t t = rk[i - 1];
        if (!(i & 3)) {
            t = lc3s_rotl(t, 8);
            t = lc3s_sbox(te, t >> 24) << 24 | lc3s_sbox(te, (t >> 16) & 255u) << 16 | lc3s_sbox(te, (t >> 8) & 255u) << 8 | lc3s_sbox(te, t & 255u);
            t ^= rc << 24;
            rc = lc3s_xtime(rc);
        }
        rk[i] = rk[i - 4] ^ t;
    }
}
/* FIPS-197 5.1 on big-endian column words: (i0 .. i3) -> (*o0 .. *o3) under the round keys rk */
static inline LC3S_HD LC3S_INL void lc3s_aes(const uint32_t* te, int nt, const uint32_t* rk, uint32_t i0, uint32_t i1, uint32_t i2, uint32_t i3, uint32_t* o0, uint32_t* o1,
                                    uint32_t* o2, uint32_t* o3)
{
    uint32_t s0 = i0 ^ rk[0], s1 = i1 ^ rk[1], s2 = i2 ^ rk[2], s3 = i3 ^ rk[3];
    for (int r = 1; r < 10; r++) {
        const uint32_t* k = rk + 4 * r;
        const uint32_t t0 = lc3s_te(te, nt, 0, s0 >> 24) ^ lc3s_te(te, nt, 1, (s1 >> 16) & 255u) ^ lc3s_te(te, nt, 2, (s2 >> 8) & 255u) ^ lc3s_te(te, nt, 3, s3 & 255u) ^ k[0];
        const uint32_t t1 = lc3s_te(te, nt, 0, s1 >> 24) ^ lc3s_te(te, nt, 1, (s2 >> 16) & 255u) ^ lc3s_te(te, nt, 2, (s3 >> 8) & 255u) ^ lc3s_te(te, nt, 3, s0 & 255u) ^ k[1];
        const uint32_t t2 = lc3s_te(te, nt, 0, s2 >> 24) ^ lc3s_te(te, nt, 1, (s3 >> 16) & 255u) ^ lc3s_te(te, nt, 2, (s0 >> 8) & 255u) ^ lc3s_te(te, nt, 3, s1 & 255u) ^ k[2];
        const uint32_t t3 = lc3s_te(te, nt, 0, s3 >> 24) ^ lc3s_te(te, nt, 1, (s0 >> 16) & 255u) ^ lc3s_te(te, nt, 2, (s1 >> 8) & 255u) ^ lc3s_te(te, nt, 3, s2 & 255u) ^ k[3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    const uint32_t* k = rk + 40;
    *o0 = (lc3s_sbox(te, s0 >> 24) << 24 | lc3s_sbox(te, (s1 >> 16) & 255u) << 16 | lc3s_sbox(te, (s2 >> 8) & 255u) << 8 | lc3s_sbox(te, s3 & 255u)) ^ k[0];
    *o1 = (lc3s_sbox(te, s1 >> 24) << 24 | lc3s_sbox(te, (s2 >> 16) & 255u) << 16 | lc3s_sbox(te, (s3 >> 8) & 255u) << 8 | lc3s_sbox(te, s0 & 255u)) ^ k[1];
    *o2 = (lc3s_sbox(te, s2 >> 24) << 24 | lc3s_sbox(te, (s3 >> 16) & 255u) << 16 | lc3s_sbox(te, (s0 >> 8) & 255u) << 8 | lc3s_sbox(te, s1 & 255u)) ^ k[2];
    *o3 = (lc3s_sbox(te, s3 >> 24) << 24 | lc3s_sbox(te, (s0 >> 16) & 255u) << 16 | lc3s_sbox(te, (s1 >> 8) & 255u) << 8 | lc3s_sbox(te, s2 & 255u)) ^ k[3];
}

/* ---- SHA-1 ---- */
/* FIPS 180-4 6.1.2: one 64-byte block w (sixteen big-endian words, used up as the schedule) into the state h.  On the device the 80 rounds are unrolled, so
 * that every index into w is a constant and the schedule stays in registers */
static inline LC3S_HD LC3S_INL void lc3s_sha1(uint32_t h[5], uint32_t w[16])
{
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
    LC3S_UNROLL
    for (int t = 0; t < 80; t++) {
        if (t >= 16) w[t & 15] = lc3s_rotl(w[(t + 13) & 15] ^ w[(t + 8) & 15] ^ w[(t + 2) & 15] ^ w[t & 15], 1);
        const uint32_t f = t < 20 ? (d ^ (b & (c ^ d))) : t < 40 ? (b ^ c ^ d) : t < 60 ? ((b & c) | (d & (b | c))) : (b ^ c ^ d);
        const uint32_t k = t < 20 ? 0x5A827999u : t < 40 ? 0x6ED9EBA1u : t < 60 ? 0x8F1BBCDCu : 0xCA62C1D6u;
        const uint32_t x = lc3s_rotl(a, 5) + f + e + k + w[t & 15];
        e = d; d = c; c = lc3s_rotl(b, 30); b = a; a = x;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}
static inline LC3S_HD void lc3s_sha1_start(uint32_t h[5]) { h[0] = 0x67452301u; h[1] = 0xEFCDAB89u; h[2] = 0x98BADCFEu; h[3] = 0x10325476u; h[4] = 0xC3D2E1F0u; }

/* ---- a packet's bytes ---- */
/* A packet at address p is read as the aligned words that hold its bytes: `base` is p rounded down to a word and sh = p & 3 on the device; on the host base is
 * p itself and sh is 0.  lc3s_aw(base, j, end) is word j behind base as it lies in memory (byte 0 lowest), 0 where it holds none of the bytes in front of `end`
 * (= sh + the packet's length, counted from base); the host reads only the bytes in front of `end` of it. */
#if defined(__HIP_DEVICE_COMPILE__)
static inline __device__ uint32_t lc3s_align(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
static inline __device__ uint32_t lc3s_bswap(uint32_t v) { return __builtin_amdgcn_perm(0, v, 0x00010203u); }
static inline __device__ const uint8_t* lc3s_base(const uint8_t* p, uint32_t* sh) { *sh = (uint32_t)((uintptr_t)p & 3); return p - *sh; }
static inline __device__ uint32_t lc3s_aw(const uint8_t* base, int j, int end) { return 4 * j < end ? *(const uint32_t*)(base + 4 * (long long)j) : 0u; }
static inline __device__ void lc3s_store(uint8_t* a, uint32_t v) { *(uint32_t*)a = v; }
#else
static inline uint32_t lc3s_align(uint32_t hi, uint32_t lo, uint32_t sh) { return sh ? hi << (32 - 8 * sh) | lo >> (8 * sh) : lo; }
static inline uint32_t lc3s_bswap(uint32_t v) { return v >> 24 | (v >> 8 & 0xFF00u) | (v << 8 & 0xFF0000u) | v << 24; }
static inline const uint8_t* lc3s_base(const uint8_t* p, uint32_t* sh) { *sh = 0; return p; }
static inline uint32_t lc3s_aw(const uint8_t* base, int j, int end)
{
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) if (4 * j + b < end) v |= (uint32_t)base[4 * (long long)j + b] << (8 * b);
    return v;
}
static inline void lc3s_store(uint8_t* a, uint32_t v) { for (int b = 0; b < 4; b++) a[b] = (uint8_t)(v >> (8 * b)); }
#endif

/* Where a walk stores: d is the address of the packet's byte 0 and [lo, hi) the bytes of the packet that may be written.  The packet's words come in one by
 * one (lc3s_put), each as it lies in memory; the sink realigns them to the words of memory and stores a whole word only where all four of its bytes lie in
 * [lo, hi), single bytes otherwise.  No word is read back, so a byte of a neighbouring packet is never written, not even with its own value. */
typedef struct { uint8_t* d; uint32_t sh, prev; int lo, hi; } lc3s_sink;
static inline LC3S_HD LC3S_INL void lc3s_sink_init(lc3s_sink* o, uint8_t* d, int lo, int hi)
{
    uint32_t sh;
    (void)lc3s_base(d, &sh);
    o->d = d; o->sh = sh; o->prev = 0; o->lo = lo; o->hi = hi;
}
/* word k of the packet (bytes 4k .. 4k + 3, byte 4k lowest); k ascends by one from call to call.  It completes the word of memory that begins sh bytes in front
 * of byte 4k */
static inline LC3S_HD LC3S_INL void lc3s_put(lc3s_sink* o, int k, uint32_t v)
{
    const uint32_t val = o->sh ? lc3s_align(v, o->prev, 4 - o->sh) : v;
    const int m0 = 4 * k - (int)o->sh;
    o->prev = v;
    if (m0 >= o->lo && m0 + 4 <= o->hi) { lc3s_store(o->d + m0, val); return; }
    for (int b = 0; b < 4; b++)
        if (m0 + b >= o->lo && m0 + b < o->hi) o->d[m0 + b] = (uint8_t)(val >> (8 * b));
}
/* behind the last word: the bytes of it that the next word of memory holds */
static inline LC3S_HD LC3S_INL void lc3s_flush(lc3s_sink* o) { lc3s_put(o, (o->hi + 3) >> 2, 0u); }

/* ---- the walk over a packet ---- */
/* A packet of L bytes whose payload begins at byte 4 * h4 (a header is a whole number of words), taken word by word as big-endian values: lc3s_next gives word k
 * with the bytes behind L zero, the payload's words XORed with the AES-CM keystream where `crypt`, and hands it to the sink where there is one.  Keystream
 * block j is AES(iv + j), one for every four payload words, kept in ks0 .. ks3. */
typedef struct {
    const uint32_t* ctx; const uint32_t* te; const uint8_t* base;
    uint32_t sh, cur, iv0, iv1, iv2, iv3, ks0, ks1, ks2, ks3;
    int L, h4, crypt, nt;
} lc3s_walk;
/* the IV of RFC 3711 4.1.1, (salt << 16) ^ (SSRC << 64) ^ (index << 16) with index = roc << 16 | seq, as four big-endian words */
static inline LC3S_HD LC3S_INL void lc3s_walk_init(lc3s_walk* w, const uint32_t* ctx, const uint32_t* te, int nt, const uint8_t* p, int L, int h4, int crypt, uint32_t ssrc,
                                          uint32_t roc, uint32_t seq, int k0)
{
    w->ctx = ctx; w->te = te; w->nt = nt; w->L = L; w->h4 = h4; w->crypt = crypt;
    w->base = lc3s_base(p, &w->sh);
    w->iv0 = ctx[LC3S_CTX_SALT]; w->iv1 = ctx[LC3S_CTX_SALT + 1] ^ ssrc; w->iv2 = ctx[LC3S_CTX_SALT + 2] ^ roc; w->iv3 = ctx[LC3S_CTX_SALT + 3] ^ seq << 16;
    w->ks0 = w->ks1 = w->ks2 = w->ks3 = 0;
    w->cur = lc3s_aw(w->base, k0, (int)w->sh + L);
}
/* word k, for 4k < L; k ascends by one from call to call, from the k0 of the init.  out: the sink, with `store` (a flag of its own: a sink's address cannot be told from NULL on the device) */
static inline LC3S_HD LC3S_INL uint32_t lc3s_next(lc3s_walk* w, lc3s_sink* out, int store, int k)
{
    const uint32_t nxt = lc3s_aw(w->base, k + 1, (int)w->sh + w->L);
    uint32_t m = lc3s_bswap(lc3s_align(nxt, w->cur, w->sh));
    w->cur = nxt;
    const uint32_t keep = 4 * k + 4 > w->L ? ~0u << (8 * (4 * k + 4 - w->L)) : ~0u;
    m &= keep;
    if (w->crypt && k >= w->h4) {
        const uint32_t pw = (uint32_t)(k - w->h4), q = pw & 3u;
        if (q == 0) lc3s_aes(w->te, w->nt, w->ctx + LC3S_CTX_RK, w->iv0, w->iv1, w->iv2, w->iv3 + (pw >> 2), &w->ks0, &w->ks1, &w->ks2, &w->ks3);
        m ^= (q == 0 ? w->ks0 : q == 1 ? w->ks1 : q == 2 ? w->ks2 : w->ks3) & keep;
    }
    if (store) lc3s_put(out, k, lc3s_bswap(m));
    return m;
}
/* the payload alone, words h4 .. : encrypts or decrypts it into the sink (the walk was begun at k0 = h4) */
static inline LC3S_HD LC3S_INL void lc3s_crypt(lc3s_walk* w, lc3s_sink* out)
{
    for (int k = w->h4; 4 * k < w->L; k++) (void)lc3s_next(w, out, 1, k);
    lc3s_flush(out);
}
/* what the bytes behind the packet add to word k of the hashed message: the four bytes of roc, the byte 80 behind them and, in the last word (k == last), the
 * message's length in bits, the 64 bytes of the ipad block included */
static inline LC3S_HD uint32_t lc3s_tail(int k, int L, uint32_t roc, int last)
{
    uint32_t v = 0;
    for (int b = 0; b < 4; b++) {
        const int d = 4 * k + b - L;
        const uint32_t x = d >= 0 && d < 4 ? (roc >> (8 * (3 - d))) & 255u : d == 4 ? 0x80u : 0u;
        v |= x << (8 * (3 - b));
    }
    return k == last ? v | (uint32_t)(64 + L + 4) * 8u : v;
}
/* RFC 3711 4.2: HMAC-SHA1(k_a, packet || roc) from the two midstates of the context; the walk (begun at k0 = 0) delivers the packet, encrypting and storing on
 * its way where it is set up to.  tag: the 20 bytes as five big-endian words.  A packet of L bytes takes (L + 13 + 63) / 64 compressions and one for the outer
 * hash */
static inline LC3S_HD LC3S_INL void lc3s_hmac(lc3s_walk* w, lc3s_sink* out, int store, uint32_t roc, uint32_t tag[5])
{
    const int L = w->L, chunks = (L + 13 + 63) >> 6;
    uint32_t hs[5];
    for (int i = 0; i < 5; i++) hs[i] = w->ctx[LC3S_CTX_IPAD + i];
    for (int c = 0; c < chunks; c++) {
        uint32_t m[16];
        LC3S_UNROLL
        for (int i = 0; i < 16; i++) {
            const int k = 16 * c + i;
            uint32_t v = 4 * k < L ? lc3s_next(w, out, store, k) : 0u;
            if (4 * k + 4 > L) v |= lc3s_tail(k, L, roc, 16 * chunks - 1);
            m[i] = v;
        }
        lc3s_sha1(hs, m);
    }
    if (store) lc3s_flush(out);
    uint32_t m[16];
    for (int i = 0; i < 5; i++) m[i] = hs[i];
    m[5] = 0x80000000u;
    for (int i = 6; i < 15; i++) m[i] = 0;
    m[15] = (64 + 20) * 8;
    for (int i = 0; i < 5; i++) tag[i] = w->ctx[LC3S_CTX_OPAD + i];
    lc3s_sha1(tag, m);
}

/* ---- the context (host only) ---- */
/* RFC 3711 4.3.1 with key derivation rate 0: the AES-CM keystream under the master key from the IV (master_salt ^ label << 48) << 16 gives the session cipher
 * key (label 0, 16 bytes), the authentication key (label 1, 20 bytes) and the session salt (label 2, 14 bytes).  te: Te0, 256 words */
static inline void lc3s_derive(const uint32_t* te, const uint32_t mrk[44], const uint8_t master_salt[14], int label, uint8_t* out, int n)
{
    uint8_t x[16];
    for (int i = 0; i < 14; i++) x[i] = master_salt[i];
    x[7] ^= (uint8_t)label; x[14] = x[15] = 0;
    uint32_t iv[4];
    for (int i = 0; i < 4; i++) iv[i] = (uint32_t)x[4 * i] << 24 | (uint32_t)x[4 * i + 1] << 16 | (uint32_t)x[4 * i + 2] << 8 | x[4 * i + 3];
    for (int j = 0; 16 * j < n; j++) {
        uint32_t o[4];
        lc3s_aes(te, 1, mrk, iv[0], iv[1], iv[2], iv[3] + (uint32_t)j, &o[0], &o[1], &o[2], &o[3]);
        for (int b = 0; b < 16 && 16 * j + b < n; b++) out[16 * j + b] = (uint8_t)(o[b >> 2] >> (8 * (3 - (b & 3))));
    }
}
/* zeroes through a volatile pointer, so that the stores stay although nothing reads them: the master key's round keys, the session keys and the context's
 * working copy do not stay on this function's stack (lc3s_derive's keystream blocks and the plan functions' keystream words are not wiped) */
static inline void lc3s_wipe(void* p, size_t n)
{
    volatile uint8_t* v = (volatile uint8_t*)p;
    while (n--) *v++ = 0;
}
static inline void lc3s_make_context(const uint8_t master_key[16], const uint8_t master_salt[14], int32_t ctx[LC3S_CTX_WORDS])
{
    uint32_t te[LC3S_TE_WORDS], mrk[44], c[LC3S_CTX_WORDS];
    uint8_t ke[16], ka[20], ks[16];
    for (uint32_t x = 0; x < LC3S_TE_WORDS; x++) te[x] = lc3s_te0(x);
    lc3s_expand(te, master_key, mrk);
    lc3s_derive(te, mrk, master_salt, 0, ke, 16);
    lc3s_derive(te, mrk, master_salt, 1, ka, 20);
    lc3s_derive(te, mrk, master_salt, 2, ks, 14);
    ks[14] = ks[15] = 0;
    for (int i = 0; i < LC3S_CTX_WORDS; i++) c[i] = 0;
    lc3s_expand(te, ke, c + LC3S_CTX_RK);
    for (int i = 0; i < 4; i++) c[LC3S_CTX_SALT + i] = (uint32_t)ks[4 * i] << 24 | (uint32_t)ks[4 * i + 1] << 16 | (uint32_t)ks[4 * i + 2] << 8 | ks[4 * i + 3];
    for (int pad = 0; pad < 2; pad++) {                              /* the state behind the block k_a ^ 36 36 .. and behind k_a ^ 5C 5C .. */
        uint32_t m[16], *h = c + (pad ? LC3S_CTX_OPAD : LC3S_CTX_IPAD);
        const uint32_t fill = pad ? 0x5Cu : 0x36u;
        for (int i = 0; i < 16; i++) {
            m[i] = 0;
            for (int b = 0; b < 4; b++) m[i] |= ((4 * i + b < 20 ? ka[4 * i + b] : 0u) ^ fill) << (8 * (3 - b));
        }
        lc3s_sha1_start(h);
        lc3s_sha1(h, m);
    }
    for (int i = 0; i < LC3S_CTX_WORDS; i++) ctx[i] = (int32_t)c[i];
    lc3s_wipe(mrk, sizeof mrk); lc3s_wipe(c, sizeof c); lc3s_wipe(ke, sizeof ke); lc3s_wipe(ka, sizeof ka); lc3s_wipe(ks, sizeof ks);
}

/* ---- the protect rule ---- */
/* the stamp's view of the packet list, the per-route tables and the destination of a protect call (next_seq may be NULL) */
typedef struct {
    const int32_t* route; const long long* offset; const int32_t* size; const uint8_t* status;
    const uint8_t* wire; const int32_t* ctx; const int32_t* roc; const int32_t* seq_base; const int32_t* next_seq;
    uint8_t* dst;
    long long wire_capacity, dst_capacity, dst_stride;
    int32_t header_room, payload_room, n_routes, tag_len;
} lc3s_protect_in;
/* a packet's rollover counter from its distance to its route's base: fewer than 65 536 sequence numbers per route and call */
static inline LC3S_HD uint32_t lc3s_roc_at(uint32_t roc, uint32_t seq_base, uint32_t seq)
{
    const uint32_t b = seq_base & 0xFFFFu, d = (seq - b) & 0xFFFFu;
    return roc + ((b + d) >> 16);
}
/* The protect rule for packet p: -> its status and *out_size; a PROTECTED packet stands in dst + p * dst_stride as header, encrypted payload and tag */
static inline LC3S_HD int lc3s_protect(const lc3s_protect_in* q, long long p, const uint32_t* te, int nt, int32_t* out_size)
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
    if ((long long)L + q->tag_len > q->dst_stride || p >= q->dst_capacity / q->dst_stride) return LC3S_PR_OVERFLOW;
    uint32_t hw[3];
    lc3r_fetch12(q->wire, a, hw);
    const uint32_t seq = hw[0] & 0xFFFFu, ssrc = hw[2];
    const uint32_t roc = lc3s_roc_at((uint32_t)q->roc[r], (uint32_t)q->seq_base[r], seq);
    uint8_t* d = q->dst + p * q->dst_stride;
    lc3s_sink out;
    lc3s_walk w;
    uint32_t tag[5];
    lc3s_sink_init(&out, d, 0, L);
    lc3s_walk_init(&w, (const uint32_t*)q->ctx + (size_t)r * LC3S_CTX_WORDS, te, nt, q->wire + a, L, LC3R_FIXED / 4, 1, ssrc, roc, seq, 0);
    lc3s_hmac(&w, &out, 1, roc, tag);
    LC3S_UNROLL
    for (int b = 0; b < 10; b++)
        if (b < q->tag_len) d[L + b] = (uint8_t)(tag[b >> 2] >> (8 * (3 - (b & 3))));
    *out_size = L + q->tag_len;
    return LC3S_PROTECTED;
}
static inline LC3S_HD void lc3s_route_out(const lc3s_protect_in* q, int r, int32_t* next_roc)
{
    const uint32_t b = (uint32_t)q->seq_base[r] & 0xFFFFu;
    next_roc[r] = (int32_t)((uint32_t)q->roc[r] + ((b + (((uint32_t)q->next_seq[r] - (uint32_t)q->seq_base[r]) & 0xFFFFu)) >> 16));
}

/* ---- the unprotect rule ---- */
/* The two functions below restate lc3r_lookup and the header checks of lc3r_parse (lc3_rtp_shim.h), which give a stream where these need the table's place
 * and the header's length; that file stays as it is so that the RTP code object does.  Whoever changes one text changes the other: tests/test_srtp_cpu.py holds
 * lc3plus_plan_srtp_unprotect's checks 1 and 2 to lc3plus_plan_rtp_parse on the same malformed datagrams. */
/* the lower bound of ssrc in key[0 .. n) compared as uint32, as lc3r_lookup walks it: -> its place in the table, or -1 where no equal key stands there */
static inline LC3S_HD int lc3s_lookup(const int32_t* key, int n, uint32_t ssrc)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)key[mid] < ssrc) lo = mid + 1; else hi = mid;
    }
    return lo < n && (uint32_t)key[lo] == ssrc ? lo : -1;
}
/* what the checks 1 and 2 leave of an item: its source (place in the table), its header's length, SEQ and SSRC */
typedef struct { int32_t src, h, seq; uint32_t ssrc; uint8_t status; } lc3s_item;
/* the parse's checks with size - tag_len in the size's place; the P bit is not looked at */
static inline LC3S_HD lc3s_item lc3s_check(const uint8_t* ring, long long capacity, long long off, int32_t size, int tag_len, const int32_t* key, int n_ssrc)
{
    lc3s_item it = {-1, 0, 0, 0, LC3S_OK};
    if (off < 0 || size < 0 || size > LC3S_MAX_PACKET || off > capacity - size) { it.status = LC3S_RANGE; return it; }
    if (size < LC3R_FIXED + tag_len) { it.status = LC3S_SHORT; return it; }
    const int len = size - tag_len;
    uint32_t w[3];
    lc3r_fetch12(ring, off, w);
    const uint32_t b0 = w[0] >> 24, b1 = (w[0] >> 16) & 255u;
    if (b0 >> 6 != 2) { it.status = LC3S_VERSION; return it; }
    if (b1 >= 192 && b1 <= 223) { it.status = LC3S_RTCP; return it; }
    int h = LC3R_FIXED + 4 * (int)(b0 & 15u);
    if (h > len) { it.status = LC3S_HEADER; return it; }
    if (b0 & 16u) {
        if (h + 4 > len) { it.status = LC3S_HEADER; return it; }
        h += 4 + 4 * (int)lc3r_fetch_be16(ring, off + h + 2);
        if (h > len) { it.status = LC3S_HEADER; return it; }
    }
    const int s = lc3s_lookup(key, n_ssrc, w[2]);
    if (s < 0) { it.status = LC3S_UNKNOWN_SSRC; return it; }
    it.src = s; it.h = h; it.seq = (int32_t)(w[0] & 0xFFFFu); it.ssrc = w[2];
    return it;
}
/* the SEQ of the datagram at off, which passed checks 1 and 2 */
static inline LC3S_HD uint32_t lc3s_seq_at(const uint8_t* ring, long long off) { return lc3r_fetch_be16(ring, off + 2); }
/* RFC 3711 3.3.1 and Appendix A: the rollover counter guessed for seq against (roc, s_l).  *refused where the guess would be roc - 1 at roc == 0 */
static inline LC3S_HD uint32_t lc3s_guess(uint32_t roc, uint32_t s_l, uint32_t seq, int* refused)
{
    *refused = 0;
    if (s_l < 32768u) {
        if ((int32_t)seq - (int32_t)s_l > 32768) { *refused = roc == 0; return roc - 1u; }
        return roc;
    }
    return s_l - 32768u > seq ? roc + 1u : roc;
}
/* Checks 3 to 6 for an item that passed 1 and 2, against its source's state as the call found it (s_l: of a source that has not started, the SEQ of its first
 * item).  -> the status; *index: the 48-bit index, *roc its upper 32 bits.  Where the status is OK the payload is decrypted in place */
static inline LC3S_HD int lc3s_unprotect(uint8_t* ring, long long off, int32_t size, int tag_len, const lc3s_item* it, const int32_t* state, uint32_t s_l_first,
                                         const uint32_t* ctx, const uint32_t* te, int nt, long long* index)
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
    const int L = size - tag_len;
    uint8_t* p = ring + off;
    lc3s_walk w;
    uint32_t tag[5], diff = 0;
    lc3s_walk_init(&w, ctx, te, nt, p, L, it->h / 4, 0, it->ssrc, roc, (uint32_t)it->seq, 0);
    lc3s_hmac(&w, NULL, 0, roc, tag);
    LC3S_UNROLL
    for (int b = 0; b < 10; b++)
        if (b < tag_len) diff |= lc3r_fetch_byte(ring, off + L + b) ^ ((tag[b >> 2] >> (8 * (3 - (b & 3)))) & 255u);
    if (diff) return LC3S_AUTH;
    lc3s_sink out;
    lc3s_sink_init(&out, p, it->h, L);
    lc3s_walk_init(&w, ctx, te, nt, p, L, it->h / 4, 1, it->ssrc, roc, (uint32_t)it->seq, it->h / 4);
    lc3s_crypt(&w, &out);
    *index = idx;
    return LC3S_OK;
}
/* a source's state after the call: top1 is its largest accepted index + 1 (0: none was accepted), bits the window bits of its accepted items against the new
 * top (lc3s_window_bit).  in and out may be one block */
static inline LC3S_HD long long lc3s_new_top(const int32_t* state, unsigned long long top1)
{
    const long long best = (long long)top1 - 1;
    if (!(state[LC3S_FLAGS] & LC3S_STARTED)) return best;
    const long long top = (long long)(uint32_t)state[LC3S_ROC] << 16 | (long long)((uint32_t)state[LC3S_S_L] & 0xFFFFu);
    return best > top ? best : top;
}
static inline LC3S_HD unsigned long long lc3s_window_bit(const int32_t* state, unsigned long long top1, long long index)
{
    const long long delta = lc3s_new_top(state, top1) - index;
    return delta >= 0 && delta < LC3S_WINDOW ? 1ull << delta : 0ull;
}
static inline LC3S_HD void lc3s_state_out(const int32_t* in, int32_t* out, unsigned long long top1, unsigned long long bits)
{
    int32_t v[LC3S_STATE_WORDS];
    for (int k = 0; k < LC3S_STATE_WORDS; k++) v[k] = in[k];
    if (top1) {
        const long long top2 = lc3s_new_top(in, top1);
        unsigned long long win = 0;
        if (in[LC3S_FLAGS] & LC3S_STARTED) {
            const long long top = (long long)(uint32_t)in[LC3S_ROC] << 16 | (long long)((uint32_t)in[LC3S_S_L] & 0xFFFFu);
            const long long shift = top2 - top;
            win = (unsigned long long)(uint32_t)in[LC3S_WIN_LO] | (unsigned long long)(uint32_t)in[LC3S_WIN_HI] << 32;
            win = shift >= LC3S_WINDOW ? 0ull : win << shift;
        }
        win |= bits;
        v[LC3S_FLAGS] |= LC3S_STARTED; v[LC3S_ROC] = (int32_t)(uint32_t)(top2 >> 16); v[LC3S_S_L] = (int32_t)(top2 & 0xFFFF);
        v[LC3S_WIN_LO] = (int32_t)(uint32_t)win; v[LC3S_WIN_HI] = (int32_t)(uint32_t)(win >> 32);
    }
    for (int k = 0; k < LC3S_STATE_WORDS; k++) out[k] = v[k];
}
/* The workspace of an unprotect call, from its first 16-aligned byte: per source top1 (uint64) and bits (uint64), per item its accepted index or -1 (int64),
 * then per source the list index of its first item that passed checks 1 and 2 (int32) and per item its source or -1 (int32) */
static inline LC3S_HD long long lc3s_workspace_bytes(long long n_items, int n_ssrc)
{
    if (n_items <= 0 || n_items >= LC3S_MAX_ITEMS || n_ssrc <= 0) return 0;
    return 16 + 8 * (2 * (long long)n_ssrc + n_items) + 4 * ((long long)n_ssrc + n_items);
}

/* one protect call: every pointer but the struct itself is a device pointer (may be NULL: in.next_seq with next_roc) */
typedef struct {
    int32_t device, sync;
    long long max_packets;
    const long long* n_packets;
    lc3s_protect_in in;
    long long* out_offset; int32_t* out_size; uint8_t* out_status; int32_t* next_roc;
    void* hip_stream;
} lc3srtp_protect_call;
/* one unprotect call (may be NULL: status, index, stats) */
typedef struct {
    int32_t device, sync, n_ssrc, tag_len;
    long long n_items, ring_capacity;
    void* ring; const long long* dg_offsets; const int32_t* dg_sizes; const int32_t* ssrc_key; const int32_t* ctx; const int32_t* state_in; int32_t* state_out;
    int32_t* sizes_out; uint8_t* status; long long* index; int32_t* stats;
    void* workspace; long long workspace_bytes;
    void* hip_stream;
} lc3srtp_unprotect_call;

#ifdef __cplusplus
extern "C" {
#endif
/* queue the kernels on q->hip_stream; wait for them only with q->sync.  0, or 1 where nothing was queued */
int lc3srtp_protect_run(const lc3srtp_protect_call* q);
int lc3srtp_unprotect_run(const lc3srtp_unprotect_call* q);
/* launches of an SRTP kernel by this process, by the kernel's symbol name in the code object; -1 for a name the library does not hold */
long long lc3srtp_launch_count(const char* kernel);
#ifdef __cplusplus
}
#endif
#endif
