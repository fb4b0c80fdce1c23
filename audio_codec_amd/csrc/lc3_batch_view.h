/* lc3_batch_view.h -- what the packet layer (lc3_packet.c) borrows of a batch, and all it can see of one: lc3_host.c, which defines the two batch structs,
 * defines the two functions beside them; lc3_packet.c includes no definition of either struct, so reaching into a batch there does not compile.
 *
 * Of a batch: its device context (dev; decoder: which kind of context it is - lc3_shim.h has a call for each that gives the device and the context's own
 * stream), n_streams, channels and ylen (the probe's kernels size their reader by it).  No stream state, no configuration, no buffer, and not the record of
 * its last call: every call of the layer is stateless (include/lc3plus_batch.h). */
#ifndef LC3_BATCH_VIEW_H
#define LC3_BATCH_VIEW_H
#include "../../include/lc3plus_batch.h"

typedef struct { void* dev; int decoder; int n_streams; int channels; int ylen; } lc3host_view;
/* b is not NULL (the entry points refuse a NULL batch first); internal to the library, not part of its ABI */
__attribute__((visibility("hidden"))) lc3host_view lc3host_enc_view(const lc3plus_batch* b);
__attribute__((visibility("hidden"))) lc3host_view lc3host_dec_view(const lc3plus_dec_batch* b);
#endif
