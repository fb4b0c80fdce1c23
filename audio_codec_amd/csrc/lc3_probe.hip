/* lc3_probe.hip -- the frame probe's library (liblc3plus_probe_hip.so): the gfx950 kernels of lc3_probe.inc and the host code that launches them, behind the
 * C ABI of lc3_probe_shim.h.  A library of its own beside liblc3plus_hip.so, so that the codec library's code object stays what it is; lc3_host.c loads it on
 * the first lc3plus_dec_batch_probe call and hands it the batch's device, plan and per-size channel table.  It keeps no state but its launch counts. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stddef.h>
#include <atomic>

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
enum { K_SIDE = 0, K_FULL, K_FULL_G, K_COUNT };
static const char* const k_names[K_COUNT] = {"lc3_probe_side_kernel", "lc3_probe_full_kernel", "lc3_probe_full_kernel_g"};
static std::atomic<long long> k_launches[K_COUNT];

extern "C" long long lc3probe_launch_count(const char* kernel)
{
    if (!kernel) return -1;
    for (int i = 0; i < K_COUNT; i++) if (!strcmp(kernel, k_names[i])) return k_launches[i].load(std::memory_order_relaxed);
    return -1;
}

#define PCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "lc3plus_probe: %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

extern "C" int lc3probe_run(const lc3probe_call* q)
{
    if (!q || !q->plan || !q->tab || q->n_items <= 0 || q->channels < 1 || q->tab_n < 2) return 1;
    PCHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->stream;
    const uint8_t* in = (const uint8_t*)q->frames;
    int which;
    if (q->depth == LC3P_DEPTH_SIDE) {
        const long long blocks = (q->n_items + 255) / 256;
        if (blocks > 0x7fffffffLL) return 1;
        hipLaunchKernelGGL(lc3_probe_side_kernel, dim3((unsigned)blocks), dim3(256), 0, s, q->plan, q->tab, q->tab_n, in, q->capacity, q->offsets, q->num_bytes,
                           q->max_bytes, q->n_items, q->info);
        which = K_SIDE;
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
        auto k = nw_max ? lc3_probe_full_kernel : lc3_probe_full_kernel_g;
        hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(wpg * WAVE), per_wave * wpg, s, q->plan, q->tab, q->tab_n, in, q->capacity, q->offsets, q->num_bytes,
                           q->max_bytes, q->n_items, nw_max, nzw, q->info);
        which = nw_max ? K_FULL : K_FULL_G;
    }
    PCHK(hipGetLastError());
    k_launches[which]++;
    if (q->sync) PCHK(hipStreamSynchronize(s));
    return 0;
}
