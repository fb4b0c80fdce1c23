/* lc3_ingest.hip -- the packet ingest's library (liblc3plus_ingest_hip.so): the gfx950 kernels of lc3_ingest.inc and the host code that launches them, behind the
 * C ABI of lc3_ingest_shim.h.  A third library beside liblc3plus_hip.so and liblc3plus_probe_hip.so, so that the code objects of those two stay what they are;
 * lc3_host.c loads it on the first lc3plus_dec_batch_ingest call and hands it the batch's device, stream count and channel count.  It keeps no state but its
 * launch counts and allocates nothing. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stddef.h>
#include <atomic>

#include "lc3_ingest_shim.h"

#define WAVE 64
#include "lc3_ingest.inc"

/* ---- host ---- */
enum { K_FILL = 0, K_ITEM, K_STREAM, K_STATUS, K_COUNT };
static const char* const k_names[K_COUNT] = {"lc3_ingest_fill_kernel", "lc3_ingest_item_kernel", "lc3_ingest_stream_kernel", "lc3_ingest_status_kernel"};
static std::atomic<long long> k_launches[K_COUNT];

extern "C" long long lc3ingest_launch_count(const char* kernel)
{
    if (!kernel) return -1;
    for (int i = 0; i < K_COUNT; i++) if (!strcmp(kernel, k_names[i])) return k_launches[i].load(std::memory_order_relaxed);
    return -1;
}

#define ICHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "lc3plus_ingest: %s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

/* workgroups of 256 lanes for n of them, at most `cap`: the item kernels walk what is left grid-stride */
static unsigned blocks_for(long long n, long long cap)
{
    const long long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

extern "C" int lc3ingest_run(const lc3ingest_call* q)
{
    if (!q || q->n_items <= 0 || q->n_items >= LC3I_MAX_ITEMS || q->n_streams < 1 || q->channels < 1 || q->n_frames <= 0 || (q->seq_bits != 16 && q->seq_bits != 32))
        return 1;
    if (!q->stream || !q->seq || !q->offsets || !q->num_bytes || !q->base || !q->out_offsets || !q->out_num_bytes || !q->cell_item || !q->counts) return 1;
    ICHK(hipSetDevice(q->device));
    hipStream_t s = (hipStream_t)q->hip_stream;
    const long long n_cells = (long long)q->n_streams * q->n_frames;
    const unsigned item_blocks = blocks_for(q->n_items, 1 << 14);
    hipLaunchKernelGGL(lc3_ingest_fill_kernel, dim3(blocks_for(n_cells, 1 << 14)), dim3(256), 0, s, (uint32_t*)q->cell_item, n_cells, q->stats,
                       (long long)q->n_streams * LC3I_STATS_WORDS);
    ICHK(hipGetLastError());
    k_launches[K_FILL]++;
    hipLaunchKernelGGL(lc3_ingest_item_kernel, dim3(item_blocks), dim3(256), 0, s, q->stream, q->seq, q->num_bytes, q->info, q->base, q->n_items, q->n_streams,
                       q->channels, q->seq_bits, q->n_frames, (uint32_t*)q->cell_item, q->stats);
    ICHK(hipGetLastError());
    k_launches[K_ITEM]++;
    hipLaunchKernelGGL(lc3_ingest_stream_kernel, dim3((unsigned)((q->n_streams + 3) / 4)), dim3(4 * WAVE), 0, s, q->offsets, q->num_bytes, q->base, q->floor,
                       q->n_streams, q->seq_bits, q->n_frames, q->out_offsets, q->out_num_bytes, q->cell_item, q->counts, q->next_base, q->stats);
    ICHK(hipGetLastError());
    k_launches[K_STREAM]++;
    if (q->item_status) {
        hipLaunchKernelGGL(lc3_ingest_status_kernel, dim3(item_blocks), dim3(256), 0, s, q->stream, q->seq, q->num_bytes, q->info, q->base, q->n_items, q->n_streams,
                           q->channels, q->seq_bits, q->n_frames, q->cell_item, q->item_status);
        ICHK(hipGetLastError());
        k_launches[K_STATUS]++;
    }
    if (q->sync) ICHK(hipStreamSynchronize(s));
    return 0;
}
