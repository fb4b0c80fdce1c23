/* lc3_fec_xor.inc -- the XOR rule of the generic FEC on the device, shared by the FEC kernels (lc3_fec.inc) and the repair kernels (lc3_repair.inc): the realigning
 * fetch of a source's bytes and lc3fec_xor_store, which writes a destination cut as the egress cuts a copy.  Included behind lc3_fec_shim.h. */
/* The XOR rule on the device.  n bytes at byte address dst become the XOR of cnt sources, source m the len[m] bytes at base + at[m] (len < 0: none) padded with
 * zeros, and of one more, the xlen bytes at byte address xsrc - by the LANES lanes of a group, l this lane's index.  The destination is cut as the egress cuts a
 * copy (lc3e_copy_layout): 16-byte pieces stored whole, head and tail words, the at most three head and three tail bytes; whatever is stored is fetched as aligned
 * source words realigned by funnel shifts and XORed in registers.  No word is read that holds no byte of its source, no byte is written outside [dst, dst + n). */
__device__ __forceinline__ uint32_t lc3fec_src_word(uintptr_t a) { return *(const uint32_t*)a; }
/* the nv (1 ... 4) bytes at byte address s as the low bytes of a word, zeros above them */
__device__ __forceinline__ uint32_t lc3fec_src_bytes(uintptr_t s, int nv)
{
    const uintptr_t a = s & ~(uintptr_t)3;
    const int b = (int)(s & 3);
    const uint32_t w0 = lc3fec_src_word(a);
    uint32_t v = w0 >> (8 * b);
    if (b + nv > 4) v = __funnelshift_r(w0, lc3fec_src_word(a + 4), 8 * b);
    return nv < 4 ? v & ((1u << (8 * nv)) - 1u) : v;
}
/* one source's share of the word at payload offset o */
__device__ __forceinline__ uint32_t lc3fec_src_dword(uintptr_t src, int32_t len, int o)
{
    const int nv = len - o;
    return nv <= 0 ? 0u : lc3fec_src_bytes(src + (uintptr_t)o, nv < 4 ? nv : 4);
}
/* one source's share of the 16 bytes at payload offset o */
__device__ __forceinline__ uint4 lc3fec_src_piece(uintptr_t src, int32_t len, int o)
{
    const int nv = len - o;
    if (nv >= 16) {
        const uintptr_t s = src + (uintptr_t)o, a = s & ~(uintptr_t)3;
        const int sh = (int)(s & 3) * 8;
        const uint32_t w0 = lc3fec_src_word(a), w1 = lc3fec_src_word(a + 4), w2 = lc3fec_src_word(a + 8), w3 = lc3fec_src_word(a + 12);
        if (!sh) return make_uint4(w0, w1, w2, w3);
        const uint32_t w4 = lc3fec_src_word(a + 16);                 /* holds the piece's last byte exactly where sh != 0 */
        return make_uint4(__funnelshift_r(w0, w1, sh), __funnelshift_r(w1, w2, sh), __funnelshift_r(w2, w3, sh), __funnelshift_r(w3, w4, sh));
    }
    return make_uint4(lc3fec_src_dword(src, len, o), lc3fec_src_dword(src, len, o + 4), lc3fec_src_dword(src, len, o + 8), lc3fec_src_dword(src, len, o + 12));
}
template <int LANES>
__device__ __forceinline__ void lc3fec_xor_store(uintptr_t dst, int n, uintptr_t base, const long long* at, const int32_t* len, int cnt, uintptr_t xsrc, int32_t xlen,
                                                 int l)
{
    const lc3e_copy_plan c = lc3e_copy_layout(dst, n);
    const int body = c.hb + 4 * c.hd, tail = body + 16 * c.pieces;
    const int bi = l < 3 ? (l < c.hb ? l : -1) : l < 6 ? (l - 3 < c.tb ? tail + 4 * c.td + l - 3 : -1) : -1;
    const int di = l < 3 ? (l < c.hd ? c.hb + 4 * l : -1) : l < 6 ? (l - 3 < c.td ? tail + 4 * (l - 3) : -1) : -1;
    if (bi >= 0 || di >= 0) {
        uint32_t vb = 0, vd = 0;
        if (bi >= 0 && xlen > bi) vb = lc3fec_src_bytes(xsrc + (uintptr_t)bi, 1);
        if (di >= 0) vd = lc3fec_src_dword(xsrc, xlen, di);
        for (int m = 0; m < cnt; m++) {
            const int32_t ln = len[m];
            const uintptr_t s = base + (uintptr_t)at[m];
            if (bi >= 0 && ln > bi) vb ^= lc3fec_src_bytes(s + (uintptr_t)bi, 1);
            if (di >= 0) vd ^= lc3fec_src_dword(s, ln, di);
        }
        if (bi >= 0) *(uint8_t*)(dst + bi) = (uint8_t)vb;
        if (di >= 0) *(uint32_t*)(dst + di) = vd;
    }
    for (int k = l; k < c.pieces; k += LANES) {                       /* dst + body is 16-byte aligned wherever pieces > 0 */
        const int o = body + 16 * k;
        uint4 v = lc3fec_src_piece(xsrc, xlen, o);
        for (int m = 0; m < cnt; m++) {
            const uint4 u = lc3fec_src_piece(base + (uintptr_t)at[m], len[m], o);
            v.x ^= u.x; v.y ^= u.y; v.z ^= u.z; v.w ^= u.w;
        }
        *(uint4*)(dst + (uintptr_t)o) = v;
    }
}
