/* lc3_srtp.hip -- the Secure RTP library (liblc3plus_srtp_hip.so), behind the C ABI of lc3_srtp_shim.h: the suite of RFC 3711, AES-CM with HMAC-SHA1, for the
 * kernels and the launch code of lc3_srtp_suite.inc.  A sibling library (DESIGN.md "Sibling libraries"): lc3_packet.c loads it on the first call and hands it the
 * batch's device.
 *
 * SHA-1 takes sixteen words a compression, its 80 rounds unrolled over a schedule in registers.  The AES table is computed into LDS by the first 256 lanes of
 * every workgroup; LC3S_NT is the number of tables kept there, 1 (Te0, the others by rotation) in the product, 4 in a build for the comparison. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "lc3_srtp_shim.h"

#define WAVE 64

/* Te0, or Te0 .. Te3, into LDS */
static inline __device__ void lc3s_tables(uint32_t* te)
{
    if (threadIdx.x < LC3S_TE_WORDS) {
        const uint32_t v = lc3s_te0(threadIdx.x);
        te[threadIdx.x] = v;
        if (LC3S_NT == 4)
            for (int k = 1; k < 4; k++) te[k * LC3S_TE_WORDS + threadIdx.x] = v >> (8 * k) | v << (32 - 8 * k);
    }
    __syncthreads();
}

#define SIB_NAME "lc3plus_srtp"
#define SUITE_KERNEL(x) lc3_srtp_##x##_kernel
#define SUITE_ABI(x) lc3srtp_##x
#define SUITE_TAG(q) (q).tag_len
#define SUITE_TAG_OK(t) ((t) == 4 || (t) == 10)
#define SUITE_CTX_WORDS LC3S_CTX_WORDS
#define SUITE_LDS __shared__ uint32_t te[LC3S_NT * LC3S_TE_WORDS];
#define SUITE_TABLES() lc3s_tables(te)
#define SUITE_LANE(ctx) ((void)0)
#define SUITE_PROTECT(q, p, size) lc3s_protect(q, p, te, LC3S_NT, size)
#define SUITE_UNPROTECT(ring, off, size, it, state, s_l_first, ctx, index) \
    lc3s_unprotect(ring, off, size, SUITE_TAG(q), it, state, s_l_first, ctx, te, LC3S_NT, index)
#include "lc3_srtp_suite.inc"
