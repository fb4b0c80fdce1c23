/* lc3_launch.h -- what the kernels (lc3_kernels.hip and its .inc files) and the host runtime that launches them (lc3_runtime.hip) both need: launch geometry, the
 * layouts a launch is sized by, and the argument structs.  The hand-over layouts in HBM (FR_WORDS, PR_WORDS, DS_*, PK_STRIDE, WS_ROW, OV_ROW_* ...) are in lc3_plan.h,
 * which the host C code reads too.  Every constant has its one definition here; the file that uses it says what it means for its kernel. */
#ifndef LC3_LAUNCH_H
#define LC3_LAUNCH_H
#include "lc3_plan.h"

#define WAVE 64
/* frames (or channel-streams) per wave or workgroup: the grid of a launch follows from them.  Those under #ifndef are build parameters (tools/variants.sh) */
#define IMDCT_FPW 8                      /* lc3_dec_kernels.inc: frames per wave of the decoder's IMDCT */
#ifndef FRONT_FPW
#define FRONT_FPW 4                      /* lc3_enc_front.inc */
#endif
#ifndef FM_F240
#define FM_F240 4               /* frames per wave at N = 240 (FM_CAP / 240).  Measured on c4 (tools/variants.sh): 2 frames (FM_CAP 480) 130.7, 4 frames 136.4, 8 frames (FM_CAP 1920) 130.1 Mframes/s */
#endif
#ifndef PRE_FPW
#define PRE_FPW 8                        /* frames per wave of the FIR kernel */
#endif
#define PRE96_ITERS 4                    /* steps of 1 920 samples per workgroup: the 120 taps are fetched once per workgroup */
#ifndef SHAPE_FPW
#define SHAPE_FPW 4                      /* lc3_enc_rate.inc: frames per wave of the wave-per-frame shape kernel */
#endif
#define RATE_WG 4                        /* lc3_enc_rate.inc: waves (channel-streams) per workgroup of the rate kernel */
#define PK_XBUF 16                       /* lc3_enc_pack.inc: words of dynamic LDS per lane of the writer (pack_fw) */
/* lc3_util_kernels.inc: the scan of packed output, tiles of PKS_TILE frames */
#define PKS_THREADS 256
#define PKS_ITEMS 8
#define PKS_TILE (PKS_THREADS * PKS_ITEMS)
struct PkSrc { const uint16_t* fsz; const int4* pend; const lc3d_chan* chans; int channels, order, S, T; };
/* lc3_dec_parse.inc: the static LDS of a parse workgroup; the runtime sizes the workgroup (waves, padding) by what is left beside it */
struct __attribute__((aligned(16))) ParseLds {
    unsigned short cum[64 * 32 + 8];     /* spectral models: cumulative frequencies, 32 per model: 0 ... 1024 in [0, 17], 0xFFFF from there on - the symbol search needs
                                          * no bound on its probe (in a valid state low < (range >> 10) * 1024, so a probe at 17 or beyond never succeeds) */
    unsigned short tcum[18 + 144];       /* TNS order (2 x 9) and coefficient (8 x 18) models */
    unsigned char lut[4096];             /* context -> model */
    unsigned mpvq[176];                  /* MPVQ offsets A(n, k) */
    int pc[LC3D_PLAN_HEAD_WORDS];
};
#endif
