// mask_tile.hpp -- the arithmetic of cv-decoder's contrast mask for ONE 64x16 tile, shared by the kernel that writes the pixel mask
// (mask.hip: contrast_mask_kernel) and the one that only counts it per lattice block (sad_gate.hip: block_contrast_kernel,
// whose grid z is the frame of a batch; the tile functions see one frame).
//
//   Sobel(gray, CV_32F, dx=1, dy=1, ksize 5, BORDER_DEFAULT) -> threshold(> 20) -> dilate(MORPH_ELLIPSE 11x11)
//
// A workgroup of 256 threads owns a 64x16 tile of mask pixels: it stages the 78x30 luma window (halo 7 = 2 Sobel + 5 dilation) in LDS,
// runs the separable derivative ([-1,-2,0,2,1] along x, then along y), keeps the thresholded 74x26 window as ballot-packed row masks in
// LDS (mask_tile_rowbits) and resolves the ellipse with four 128-bit window extractions per pixel, rows of equal half-width OR-ed first
// (mask_tile_dilated).  Everything is force-inlined: the two kernels hold the same instructions for the shared part.
#pragma once

#include "common.hpp"

namespace ofps {

constexpr int MT_W = 64, MT_H = 16;            // mask tile
constexpr int MG_W = MT_W + 14, MG_H = MT_H + 14;   // luma window (halo 7)
constexpr int MS_W = MT_W + 10, MS_H = MT_H + 10;   // thresholded window (halo 5)

__device__ __forceinline__ int reflect101(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - p - 2;
    return p;
}

// extract bits [s, s + n) of the 128-bit row mask (lo = columns 0..63, hi = columns 64..)
__device__ __forceinline__ bool mask_any(unsigned long long lo, unsigned long long hi, int s, int n) {
    const unsigned long long v = s >= 64 ? hi >> (s - 64) : (s ? (lo >> s) | (hi << (64 - s)) : lo);
    return (v & ((1ull << n) - 1ull)) != 0ull;
}

// The thresholded window of the tile at (x0, y0) -> rowbits, one bit per column; g and hx are the workgroup's staging arrays.  Ends
// with a barrier: rowbits is ready for every thread when this returns.
__device__ __forceinline__ void mask_tile_rowbits(const uint8_t* __restrict__ gray, int W, int H, int stride, int x0, int y0,
                                                  uint8_t (&g)[MG_H][MG_W + 2], short (&hx)[MG_H][MS_W + 2],
                                                  unsigned long long (&rowbits)[MS_H][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // luma window; coordinates outside the image follow BORDER_REFLECT_101 (only consumed by Sobel taps of in-image
    // pixels: out-of-image thresholded pixels are forced to 0 below).  One column per thread, rows strided: no
    // per-element division.
    {
        constexpr int RPP = 256 / MG_W;                       // 3 rows per pass
        const int c = tid % MG_W, r0 = tid / MG_W;
        if (r0 < RPP) {
            const int xx = reflect101(x0 - 7 + c, W);
            for (int r = r0; r < MG_H; r += RPP) g[r][c] = gray[(size_t)reflect101(y0 - 7 + r, H) * stride + xx];
        }
    }
    __syncthreads();
    // d/dx: hx(r, c) for the thresholded window's columns (window col c <-> luma col c + 2)
    {
        constexpr int RPP = 256 / MS_W;                       // 3
        const int c = tid % MS_W, r0 = tid / MS_W;
        if (r0 < RPP) {
            for (int r = r0; r < MG_H; r += RPP)
                hx[r][c] = (short)(-(int)g[r][c] - 2 * (int)g[r][c + 1] + 2 * (int)g[r][c + 3] + (int)g[r][c + 4]);
        }
    }
    __syncthreads();
    // d/dy + threshold, packed by ballots: wave w owns rows w, w+4, ...; lanes = columns 0..63, then 64..73.
    // Pixels outside the image never win the dilation's max.
    for (int r = wave; r < MS_H; r += 4) {
        const int yy = y0 - 5 + r;
        const bool row_in = yy >= 0 && yy < H;
        auto thr_at = [&](int c) {
            const int s = -(int)hx[r][c] - 2 * (int)hx[r + 1][c] + 2 * (int)hx[r + 3][c] + (int)hx[r + 4][c];
            const int xx = x0 - 5 + c;
            return s > 20 && row_in && xx >= 0 && xx < W;
        };
        const unsigned long long lo = __ballot(thr_at(lane));
        const unsigned long long hi = __ballot(lane < MS_W - 64 && thr_at(64 + lane));
        if (lane == 0) { rowbits[r][0] = lo; rowbits[r][1] = hi; }
    }
    __syncthreads();
}

// the mask at tile pixel (lx, ly): dilation by the 11x11 ellipse, row half-widths cvRound(5*sqrt(1 - dy^2/25)) = {0,3,4,5,5,5,5,5,4,3,0}: rows that
// share a half-width are OR-ed first (wave-uniform when ly is), then one window extraction per half-width and lane
__device__ __forceinline__ bool mask_tile_dilated(const unsigned long long (&rowbits)[MS_H][2], int lx, int ly) {
    unsigned long long m0l = rowbits[ly][0] | rowbits[ly + 10][0], m0h = rowbits[ly][1] | rowbits[ly + 10][1];
    unsigned long long m3l = rowbits[ly + 1][0] | rowbits[ly + 9][0], m3h = rowbits[ly + 1][1] | rowbits[ly + 9][1];
    unsigned long long m4l = rowbits[ly + 2][0] | rowbits[ly + 8][0], m4h = rowbits[ly + 2][1] | rowbits[ly + 8][1];
    unsigned long long m5l = 0, m5h = 0;
#pragma unroll
    for (int i = 3; i <= 7; ++i) { m5l |= rowbits[ly + i][0]; m5h |= rowbits[ly + i][1]; }
    return mask_any(m0l, m0h, lx + 5, 1) || mask_any(m3l, m3h, lx + 2, 7) || mask_any(m4l, m4h, lx + 1, 9) ||
           mask_any(m5l, m5h, lx, 11);
}

}  // namespace ofps
