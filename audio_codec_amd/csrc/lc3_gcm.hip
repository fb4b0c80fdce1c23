/* lc3_gcm.hip -- the Secure RTP AES-GCM library (liblc3plus_gcm_hip.so), behind the C ABI of lc3_gcm_shim.h: the suites of RFC 7714 for the kernels and the
 * launch code of lc3_srtp_suite.inc.  A sibling library (DESIGN.md "Sibling libraries"): lc3_packet.c loads it on the first GCM call and hands it the batch's
 * device.
 *
 * Te0 is computed into LDS by every workgroup; round keys, salt and round count are read from the route's or source's context where it lies, so that contexts of
 * both key sizes stand side by side.  GHASH is serial inside a packet like SHA-1, 32 table steps a block.  Protect is one walk: fetch, XOR, hash the ciphertext
 * word, store.  Unprotect is two: hash without a store, compare, then decrypt into the sink.  The lanes of a wave hold different keys, so different GHASH tables:
 * every lane copies its table (256 bytes of its context) into LDS before its walk, lane-interleaved so that the lanes of a wave read 64 different banks - 64 KiB a
 * workgroup, two workgroups a CU.  With -DLC3G_LDS_TABLE=0 the table is read from the context in global memory instead, 16 bytes a step; that build measured 1.5
 * to 1.6 times slower (the comparison of DESIGN 10l, profiles/gcm_tables_ab.txt). */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "lc3_gcm_shim.h"

#define WAVE 64

/* Te0 into LDS */
static inline __device__ void lc3g_tables(uint32_t* te)
{
    if (threadIdx.x < LC3S_TE_WORDS) te[threadIdx.x] = lc3s_te0(threadIdx.x);
    __syncthreads();
}
#if LC3G_LDS_TABLE
/* word w of entry e of this lane's table goes to word (4 e + w) * 256 + lane: only this lane reads or writes it, so no barrier */
static inline __device__ void lc3g_table_in(uint32_t* gtab, const uint32_t* ctx)
{
    for (int i = 0; i < 64; i++) gtab[i * LC3S_THREADS + threadIdx.x] = ctx[LC3G_CTX_TABLE + i];
}
#define SUITE_LDS __shared__ uint32_t te[LC3S_TE_WORDS]; __shared__ uint32_t gtab[64 * LC3S_THREADS];
#define SUITE_LANE(ctx) lc3g_table_in(gtab, ctx)
#define LC3G_TAB (gtab + threadIdx.x)
#define LC3G_TS LC3S_THREADS
#else
#define SUITE_LDS __shared__ uint32_t te[LC3S_TE_WORDS];
#define SUITE_LANE(ctx) ((void)0)
#define LC3G_TAB ((const uint32_t*)0)
#define LC3G_TS 1
#endif

#define SIB_NAME "lc3plus_gcm"
#define SUITE_KERNEL(x) lc3_gcm_##x##_kernel
#define SUITE_ABI(x) lc3gcm_##x
#define SUITE_TAG(q) LC3G_TAG_BYTES
#define SUITE_TAG_OK(t) ((t) == LC3G_TAG_BYTES)
#define SUITE_CTX_WORDS LC3G_CTX_WORDS
#define SUITE_TABLES() lc3g_tables(te)
#define SUITE_PROTECT(q, p, size) lc3g_protect(q, p, te, 1, LC3G_TAB, LC3G_TS, size)
#define SUITE_UNPROTECT(ring, off, size, it, state, s_l_first, ctx, index) \
    lc3g_unprotect(ring, off, size, it, state, s_l_first, ctx, te, 1, LC3G_TAB, LC3G_TS, index)
#include "lc3_srtp_suite.inc"
