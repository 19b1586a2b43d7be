// jamun_conv_mf_layout.h — workgroup size and LDS layout (byte offsets) shared by the matrix-formed convs (jamun_conv_mf.hip) and the
// tail-tile kernels (jamun_conv_tail.hip), which form against the same resident x^T window and coefficient tiles.
#pragma once

#define MF_THREADS 512
#define MF_ROWB 144                      // bytes per row of a K = 64 plane of halves: 128 + 16 (rows 16 B apart mod 256: conflict-free b128 reads)
#define MF_X0H 0                         // [128 channels][64 j] hi | lo
#define MF_X0L (128 * MF_ROWB)
#define MF_X1H (2 * 128 * MF_ROWB)       // [3 m][32 u][64 j] hi | lo
#define MF_X1L (MF_X1H + 96 * MF_ROWB)
#define MF_TT (MF_X1L + 96 * MF_ROWB)    // [2 buffers][hi, lo][32 w'][64 j]
#define MF_TTB (2 * 32 * MF_ROWB)
#define MF_C (MF_TT + 2 * MF_TTB)        // [2 buffers][4 components][hi, lo][32 i][64 j]
#define MF_CB (4 * 2 * 32 * MF_ROWB)
#define MF_MISC (MF_C + 2 * MF_CB)       // deg[32] | xmax
#define MF_LDS_BYTES (MF_MISC + 144)
#define MF_PL (32 * MF_ROWB)             // hi -> lo plane of a T / C tile
