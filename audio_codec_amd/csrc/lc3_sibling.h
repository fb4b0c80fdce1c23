/* lc3_sibling.h -- what the host half of every sibling library (lc3_probe.hip ... lc3_srtp.hip; DESIGN.md "Sibling libraries") shares: the error check, the grid
 * size, and the launch that counts itself.  Host-only C++, no device code.  Included behind the library's kernels, with SIB_NAME the prefix of its messages:
 *     #define SIB_NAME "lc3plus_probe"
 *     #include "lc3_sibling.h"
 *     static const sib_kernel k_table[] = {SIB_KERNEL(lc3_probe_side_kernel), ...};
 *     extern "C" long long lc3probe_launch_count(const char* kernel) { return sib_launch_count(k_table, kernel); } */
#ifndef LC3_SIBLING_H
#define LC3_SIBLING_H
#ifndef SIB_NAME
#error "define SIB_NAME (the prefix of the library's messages on stderr) before lc3_sibling.h"
#endif
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <atomic>

/* inside a function that returns 0 or 1: a failed HIP call is said on stderr and ends it with 1 */
#define SIB_CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, SIB_NAME ": %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

/* workgroups of `threads` lanes for n lanes of work, at least one and at most `most`: the kernels walk the rest grid-stride */
static inline unsigned sib_blocks_for(long long n, int threads, long long most)
{
    const long long b = (n + threads - 1) / threads;
    return (unsigned)(b < 1 ? 1 : b > most ? most : b);
}

/* One launch counter per kernel, found by the kernel itself: a launch cannot forget its count, and the name a count is asked for under (SIB_KERNEL) is the
 * kernel's identifier. */
template <auto Kernel> static std::atomic<long long> sib_launches;
struct sib_kernel { const char* name; const std::atomic<long long>* launches; };
#define SIB_KERNEL(kernel) {#kernel, &sib_launches<kernel>}
/* hipLaunchKernelGGL's arguments; launches, checks and counts */
#define SIB_LAUNCH(kernel, ...) do { hipLaunchKernelGGL(kernel, __VA_ARGS__); SIB_CHK(hipGetLastError()); sib_launches<kernel>++; } while (0)

/* launches of the table's kernel of that name so far; -1 for a name that is not in the table */
template <int N> static inline long long sib_launch_count(const sib_kernel (&table)[N], const char* kernel)
{
    if (!kernel) return -1;
    for (int i = 0; i < N; i++) if (!strcmp(kernel, table[i].name)) return table[i].launches->load(std::memory_order_relaxed);
    return -1;
}
#endif
