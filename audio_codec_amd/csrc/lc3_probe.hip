/* lc3_probe.hip -- the frame probe's library (liblc3plus_probe_hip.so): the gfx950 kernels of lc3_probe.inc and the host code that launches them, behind the
 * C ABI of lc3_probe_shim.h.  A sibling library (DESIGN.md "Sibling libraries"): lc3_packet.c loads it on the first lc3plus_dec_batch_probe call and hands it the
 * batch's device, plan and per-size channel table.  It keeps no state but its launch counts. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#define LC3T_QUAL static __device__ const
#include "lc3_tables.h"
#include "lc3_plan.h"
#include "lc3_probe_shim.h"

#define WAVE 64
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int ilog2(unsigned v) { return 31 - __clz((int)v); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
/* floor(log2f((float)v)) as glibc evaluates it (lc3_kernels.hip flog2f_int): log2f rounds to an integer for the few v just below 2^b */
__device__ __forceinline__ int flog2f_int(unsigned v)
{
    int e = ilog2(v);
    if (v >= (1u << 20)) {
        const int b = e + 1;
        const unsigned k = (1u << b) - v;
        if ((b == 21 && k <= 1) || (b == 22 && k <= 2) || (b == 23 && k <= 5) || (b == 24 && k <= 11)) e = b;
    }
    return e;
}

#include "lc3_probe.inc"

/* ---- host ---- */
#define SIB_NAME "lc3plus_probe"
#include "lc3_sibling.h"
static const sib_kernel k_table[] = {SIB_KERNEL(lc3_probe_side_kernel), SIB_KERNEL(lc3_probe_full_kernel), SIB_KERNEL(lc3_probe_full_kernel_g)};
extern "C" long long lc3probe_launch_count(const char* kernel) { return sib_launch_count(k_table, kernel); }

extern "C" int lc3probe_run(const lc3probe_call* q)
{
    if (!q || !q->plan || !q->tab || q->n_items <= 0 || q->channels < 1 || q->tab_n < 2) return 1;
    SIB_CHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->stream;
    const uint8_t* in = (const uint8_t*)q->frames;
    if (q->depth == LC3P_DEPTH_SIDE) {
        const long long blocks = (q->n_items + 255) / 256;
        if (blocks > 0x7fffffffLL) return 1;
        SIB_LAUNCH(lc3_probe_side_kernel, dim3((unsigned)blocks), dim3(256), 0, s, q->plan, q->tab, q->tab_n, in, q->capacity, q->offsets, q->num_bytes,
                   q->max_bytes, q->n_items, q->info);
    } else {
        /* the host does not see the sizes: a channel holds at most its share of max_bytes, and at most the geometry's largest channel frame (as the parser of
         * decode_packed bounds them).  Up to 128 bytes the channel is staged in LDS; above that four waves' worth would not fit beside the tables */
        const int share = (q->max_bytes + q->channels - 1) / q->channels;
        const int max_nb = share < q->tab_n - 1 ? share : q->tab_n - 1;
        const int nw_max = max_nb > 128 ? 0 : (max_nb + 3) / 4;
        const int nzw = (q->ylen / 2 + 15) / 16;                        /* two bits per tuple */
        const size_t per_wave = (size_t)(nw_max + nzw) * WAVE * sizeof(unsigned);
        int wpg = (int)((64 * 1024 - sizeof(ProbeLds)) / per_wave);
        if (wpg > 4) wpg = 4;
        if (wpg < 1) return 1;
        const long long per_wg = (long long)wpg * WAVE, blocks = (q->n_items + per_wg - 1) / per_wg;
        if (blocks > 0x7fffffffLL) return 1;
#define FULL_ARGS dim3((unsigned)blocks), dim3(wpg * WAVE), per_wave * wpg, s, q->plan, q->tab, q->tab_n, in, q->capacity, q->offsets, q->num_bytes, q->max_bytes, q->n_items, \
                  nw_max, nzw, q->info
        if (nw_max) SIB_LAUNCH(lc3_probe_full_kernel, FULL_ARGS);
        else SIB_LAUNCH(lc3_probe_full_kernel_g, FULL_ARGS);
#undef FULL_ARGS
    }
    if (q->sync) SIB_CHK(hipStreamSynchronize(s));
    return 0;
}
