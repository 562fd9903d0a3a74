// flux_blur_kernels.hip - the convolved sun: one Gaussian window per bitmap, given by its covariance in pixels^2 (gfx950).
//
// The blur mode of art_flux_crop_fwd (include/artist_hip.h).  Per bitmap b with covariance (Srr, Src, Scc), r = row, c = column:
//   column pass       y[r,c] = sum_k g_a[k]   x[r, c - k],               a = Scc - Src^2 / Srr
//   sheared row pass  z[r,c] = sum_k g_Srr[k] lerp(y[r - k, .], c - s k), s = Src / Srr
// g_v[k], k = -K..K, K = ceil(4 sqrt(v)), are exp(-k^2 / (2 v)) over their sum (one tap of weight 1 when v < 1e-4).  x is zero
// outside the image, y is kept BEYOND the image's edges and z is cut to the image: zero-extend, convolve with a point-symmetric
// stencil, restrict - so the operator is its own adjoint and the backward pass is this kernel on the upstream gradient.
//
// One kernel, no workspace.  A workgroup owns an output tile that is a PARALLELOGRAM: TR rows, and in row r0 + i the 64 columns
// from c0 + sh(i), sh(d) = floor(s d) in 16.16 fixed point - the tile leans the way the window does.  The rows of y that its row
// pass reads, r0 - Kr .. r0 + TR - 1 + Kr, lean with it (row r0 + d is kept from column c0 + sh(d) - 2), so every one of them is
// 68 columns wide whatever the shear and the radius, tiles that are as tall as the image fit LDS (TR = 256 at the bench's size),
// and a row of y is computed by one tile column only - not once per tile that a rectangular tiling would stack on it.
// Column pass: a wave takes 2 rows of y per round; their x rows (68 + 2 Ka columns, zero outside the image) are staged in the
// wave's LDS strips, the next round's are in flight in registers meanwhile; a round whose x rows are all zero writes zeros and
// skips its taps.  Row pass out of LDS: wave w owns 8 consecutive rows of each block of 128, lane l column c0 + sh(i) + l; rows and tiles
// that lie outside the image (the parallelograms' corners) are skipped, and so are the taps into rows of y whose input was all zero.
// The tiling, the tables and the order of every sum depend on the bitmap's own covariance and on (Hh, W) alone: a bitmap's bits
// depend neither on B, nor on its place in the batch, nor on the run.  No atomics.  Taps are summed in ascending k.
// (Below the forward: flux_blur_grad_kernel, the gradient with respect to the covariance - the blur mode of art_flux_crop_bwd.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "launch_common.hpp"

namespace art {

constexpr int kBlurBlock = 1024;                // 16 waves: one workgroup per CU (the LDS image), 4 waves per SIMD to hide LDS latency
constexpr int kBlurWaves = kBlurBlock / 64;
constexpr int kBlurTileCols = 64;               // = the wave: lane l owns a column, consecutive lanes read consecutive banks
constexpr int kBlurMaxTileRows = 256;
constexpr int kBlurMinTileRows = 8;
constexpr int kBlurMaxRadius = 64;              // taps -64..64 per pass: THE limit of the operator (4 sqrt(v) <= 64)
constexpr int kBlurTaps = 2 * kBlurMaxRadius + 1;
constexpr int kBlurRowsPerWave = 8;             // consecutive output rows per wave in a block of 128 tile rows
constexpr int kBlurTailCols = 4;
constexpr int kBlurImageCols = kBlurTileCols + kBlurTailCols;    // columns of a row of y in LDS: 68, what a tile row's taps reach (see the row pass)
constexpr int kBlurRound = 2;                   // rows of y per wave and round of the column pass
constexpr int kBlurPrefetch = 4;                // x columns per lane and row in flight: a row of 68 + 2 * 64 <= 256 columns
constexpr int kBlurStrip = kBlurImageCols + 2 * kBlurMaxRadius + 2;                  // floats per x strip: 198
constexpr int kBlurLdsFloats = (kBlurMaxTileRows + 2 * kBlurMaxRadius) * kBlurImageCols + kBlurWaves * kBlurRound * kBlurStrip;   // 129,792 B
constexpr double kBlurMinVariance = 1e-4;       // below: the pass is the identity
constexpr double kBlurPsdSlack = 1e-5;          // Src^2 <= Srr Scc (1 + slack): fp32 rounding of a rank-deficient J C J^T

struct BlurPlan {          // the same in every thread of every workgroup of a bitmap
    int valid;             // 0: the bitmap is NaN
    int Kr, Ka;            // radii of the row and the column pass
    int TR;                // rows per tile
    int smin, smax;        // range of sh(i) over a tile's rows
    int sfix, sbits;       // round(s * 2^sbits): 16 bits, 10 for |s| > 64 (sfix * d stays an int for |d| < 512 either way)
    double Srr, s, a;
};

__device__ static BlurPlan blur_plan(const float* __restrict__ cov, int Hh)
{
    BlurPlan p;
    const double Srr = (double)cov[0], Src = (double)cov[1], Scc = (double)cov[2];
    p.valid = 0; p.Kr = p.Ka = 0; p.TR = kBlurMinTileRows; p.smin = p.smax = 0; p.sfix = 0; p.sbits = 16;
    p.Srr = Srr; p.s = 0.0; p.a = Scc;
    const double radius2 = (double)(kBlurMaxRadius * kBlurMaxRadius) / 16.0;      // 4 sqrt(v) <= 64
    if (!(isfinite(Srr) && isfinite(Src) && isfinite(Scc))) return p;
    if (!(Srr >= 0.0 && Scc >= 0.0 && Src * Src <= Srr * Scc * (1.0 + kBlurPsdSlack))) return p;
    if (!(Srr <= radius2 && Scc <= radius2)) return p;
    if (Srr >= kBlurMinVariance) {
        p.Kr = (int)ceil(4.0 * sqrt(Srr));
        p.s = Src / Srr;
        p.a = Scc - Src * Src / Srr;
    }
    if (p.a >= kBlurMinVariance) p.Ka = (int)ceil(4.0 * sqrt(p.a));
    // (|s| <= sqrt(Scc / Srr) <= 1600 for what passed the checks above; the bound keeps sfix an int)
    if (p.Kr > kBlurMaxRadius || p.Ka > kBlurMaxRadius || !(fabs(p.s) <= 4096.0)) return p;
    int TR = kBlurMinTileRows;
    while (TR < kBlurMaxTileRows && TR < Hh) TR <<= 1;
    p.TR = TR;
    p.sbits = fabs(p.s) <= 64.0 ? 16 : 10;
    p.sfix = (int)llrint(p.s * (double)(1 << p.sbits));
    const int last = (p.sfix * (TR - 1)) >> p.sbits;
    p.smin = min(0, last);
    p.smax = max(0, last);
    p.valid = 1;
    return p;
}

// Normalised weights of one pass into w[0 .. 2K], by ONE wave: lane l holds exp(-(l+1)^2 / (2 v)), the sum is a butterfly in fp64.
__device__ __forceinline__ void blur_weights(double v, int K, int lane, float* __restrict__ w)
{
    const int k = lane + 1;
    const double e = k <= K ? exp(-(double)(k * k) / (2.0 * v)) : 0.0;
    double sum = e;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const double total = 1.0 + 2.0 * sum;
    if (lane == 0) w[K] = (float)(1.0 / total);
    if (k <= K) {
        w[K + k] = (float)(e / total);
        w[K - k] = (float)(e / total);
    }
}

// sh(d): how far row r0 + d of a tile leans, in columns (the SAME integer wherever a row's place is needed).
__device__ __forceinline__ int blur_shear(const BlurPlan& p, int d) { return (p.sfix * d) >> p.sbits; }

// Entry `index` (the same in every lane, < 64) of a table that the wave holds one entry per lane: no LDS round trip in a tap loop.
__device__ __forceinline__ float blur_lane_f(float table, int index)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(table), index));
}

// The row pass for the wave's NR consecutive rows i0 + m, m < NR.
// Output (i, l) is column c = c0 + sh(i) + l; tap k reads row d = i - k of y at columns c + o_k and the next one, o_k = floor(-s k):
// in that row's LDS image, which starts at c0 + sh(d) - 2, that is l + e and l + e + 1 with e = sh(i) - sh(d) + o_k + 2 in 0..3
// (sh(i) - sh(d) is within 1 of s k, o_k within 1 below -s k).  The address is a sum of three byte offsets: row_offset[d + Kr] =
// 4 ((d + Kr) 68 - sh(d) + 2), a table in LDS (the CU's one scalar unit cannot form sh(d) for every row and tap); lane_term[m] =
// 4 (sh(i) + l); and 4 o_k.
//
// Taps t0 .. t1 - 1 (inside the segment of 64 table entries that starts at `segment`), one table read per row and tap.
// CLAMPED: the wave holds rows past the run's end; they repeat the run's last row (row_of[m] = min(i, iz - 1)) and are not stored,
// so that every read stays inside the tile's image of y.
template <int NR, bool CLAMPED>
__device__ __forceinline__ void blur_row_taps(float (&acc)[NR], const int (&lane_term)[NR], const int (&row_of)[NR], float tw, float tf,
                                              int to, int segment, int t0, int t1, int i0, int Kr, const int* __restrict__ row_offset,
                                              const float* __restrict__ Y)
{
    for (int t = t0; t < t1; ++t) {
        const float w = blur_lane_f(tw, t - segment);
        const float f = blur_lane_f(tf, t - segment);
        const int o4 = 4 * __builtin_amdgcn_readlane(to, t - segment);
        const int* __restrict__ rows = row_offset + (i0 - (t - Kr) + Kr);      // |k| <= Kr: d + Kr >= 0
#pragma unroll
        for (int m = 0; m < NR; ++m) {
            const int row = CLAMPED ? row_offset[row_of[m] - (t - Kr) + Kr] : rows[m];
            const float* __restrict__ yr = reinterpret_cast<const float*>(reinterpret_cast<const char*>(Y) + (row + lane_term[m] + o4));
            const float v0 = yr[0], v1 = yr[1];
            acc[m] = __builtin_fmaf(w, __builtin_fmaf(f, v1 - v0, v0), acc[m]);
        }
    }
}

// NR taps t .. t + NR - 1 (inside one segment) at once: row m at tap t + u reads row i0 + m - u + 2 Kr - t of y, so the NR x NR
// (row, tap) pairs share 2 NR - 1 table entries, read once into registers - the same sums in the same order as tap by tap.
template <int NR>
__device__ __forceinline__ void blur_row_tap_block(float (&acc)[NR], const int (&lane_term)[NR], float tw, float tf, int to, int segment,
                                                   int t, int i0, int Kr, const int* __restrict__ row_offset, const float* __restrict__ Y)
{
    const int* __restrict__ rows = row_offset + (i0 + 2 * Kr - t - (NR - 1));      // t + NR - 1 <= 2 Kr: the first index is >= i0
    int row[2 * NR - 1];
#pragma unroll
    for (int q = 0; q < 2 * NR - 1; ++q) row[q] = rows[q];
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        const float w = blur_lane_f(tw, t + u - segment);
        const float f = blur_lane_f(tf, t + u - segment);
        const int o4 = 4 * __builtin_amdgcn_readlane(to, t + u - segment);
#pragma unroll
        for (int m = 0; m < NR; ++m) {
            const float* __restrict__ yr =
                reinterpret_cast<const float*>(reinterpret_cast<const char*>(Y) + (row[m - u + NR - 1] + lane_term[m] + o4));
            const float v0 = yr[0], v1 = yr[1];
            acc[m] = __builtin_fmaf(w, __builtin_fmaf(f, v1 - v0, v0), acc[m]);
        }
    }
}

// Taps t0 .. t1 - 1 of the column pass for the round's 2 rows: y column i reads x column i - k = strip[i + 2 Ka - t].
__device__ __forceinline__ void blur_column_taps(float (&acc)[kBlurRound], float& tail, float tw, int t0, int t1, int Ka,
                                                 const float* __restrict__ xs, const float* __restrict__ xt)
{
    for (int t = t0; t < t1; ++t) {
        const float w = blur_lane_f(tw, t - t0);
        const int q0 = 2 * Ka - t;
#pragma unroll
        for (int q = 0; q < kBlurRound; ++q) acc[q] = __builtin_fmaf(w, xs[q * kBlurStrip + q0], acc[q]);
        tail = __builtin_fmaf(w, xt[q0], tail);
    }
}

// The x rows under the round's rows j, j + 1 of a tile's image of y, columns (c0 + sh(j - Kr) - 2) - Ka and the 68 + 2 Ka - 1 after it, zero
// outside the image: into registers.
__device__ __forceinline__ void blur_fetch_rows(const float* __restrict__ xb, const BlurPlan& p, int r0, int c0, int j, int rows_y, int Hh,
                                                int W, int Wx, int lane, float (&pre)[kBlurRound][kBlurPrefetch])
{
#pragma unroll
    for (int q = 0; q < kBlurRound; ++q) {
        const int r = r0 + j + q - p.Kr;
        const bool live = j + q < rows_y && r >= 0 && r < Hh;
        const int first = c0 + blur_shear(p, j + q - p.Kr) - 2 - p.Ka;
        const float* __restrict__ xr = xb + (size_t)(live ? r : 0) * (size_t)W;
#pragma unroll
        for (int u = 0; u < kBlurPrefetch; ++u) {
            const int i = lane + 64 * u;
            const int c = first + i;
            pre[q][u] = (live && i < Wx && c >= 0 && c < W) ? xr[c] : 0.0f;
        }
    }
}

__global__ __launch_bounds__(kBlurBlock) void flux_blur_kernel(const float* __restrict__ x, const float* __restrict__ cov, int Hh, int W,
                                                               float* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float blur_lds[];
    __shared__ float s_wr[kBlurTaps], s_fr[kBlurTaps], s_wa[kBlurTaps];
    __shared__ int s_or[kBlurTaps];
    __shared__ int s_row[kBlurMaxTileRows + 2 * kBlurMaxRadius];      // see blur_row_taps
    __shared__ int s_live[(kBlurMaxTileRows + 2 * kBlurMaxRadius) / kBlurRound];     // per round of the column pass: any input non-zero

    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t image = (size_t)b * (size_t)Hh * (size_t)W;
    const float* __restrict__ xb = x + image;
    float* __restrict__ ob = out + image;
    BlurPlan p = blur_plan(cov + 3 * (size_t)b, Hh);
    // (the plan is the same in every lane, but it comes out of fp64 vector arithmetic: tell the compiler, so that row indices,
    //  loop bounds and branches on it are scalar)
    p.valid = __builtin_amdgcn_readfirstlane(p.valid);
    p.Kr = __builtin_amdgcn_readfirstlane(p.Kr);
    p.Ka = __builtin_amdgcn_readfirstlane(p.Ka);
    p.TR = __builtin_amdgcn_readfirstlane(p.TR);
    p.smin = __builtin_amdgcn_readfirstlane(p.smin);
    p.smax = __builtin_amdgcn_readfirstlane(p.smax);
    p.sfix = __builtin_amdgcn_readfirstlane(p.sfix);
    p.sbits = __builtin_amdgcn_readfirstlane(p.sbits);

    if (!p.valid) {         // marked in the result itself: the whole bitmap is NaN
        const size_t n = (size_t)Hh * (size_t)W;
        for (size_t i = (size_t)blockIdx.x * kBlurBlock + tid; i < n; i += (size_t)gridDim.x * kBlurBlock) ob[i] = __builtin_nanf("");
        return;
    }

    const int Kr = p.Kr, Ka = p.Ka, TR = p.TR;
    constexpr int Wy = kBlurImageCols;
    const int rows_y = TR + 2 * Kr;
    const int Wx = Wy + 2 * Ka;
    float* __restrict__ Y = blur_lds;                                                              // [rows_y][Wy]
    float* __restrict__ strips = blur_lds + (kBlurMaxTileRows + 2 * kBlurMaxRadius) * Wy + wave * kBlurRound * kBlurStrip;

    if (wave == 0) blur_weights(p.Srr, Kr, lane, s_wr);
    if (wave == 1) blur_weights(p.a, Ka, lane, s_wa);
    if (tid >= 128 && tid < 128 + 2 * Kr + 1) {     // where tap k of the row pass reads: column c + floor(-s k), fraction of -s k
        const int k = tid - 128 - Kr;
        const double pos = -p.s * (double)k;
        const double fl = floor(pos);
        s_or[tid - 128] = (int)fl;
        s_fr[tid - 128] = (float)(pos - fl);
    }
    for (int j = tid; j < kBlurMaxTileRows + 2 * kBlurMaxRadius; j += kBlurBlock) s_row[j] = 4 * (j * Wy - blur_shear(p, j - Kr) + 2);
    __syncthreads();
    // the tables, one entry per lane and segment of 64 taps (2 K + 1 <= 129 entries: three segments)
    float wr[3], fr[3], wa[3];
    int orr[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int t = lane + 64 * g;
        wr[g] = t <= 2 * Kr ? s_wr[t] : 0.0f;
        fr[g] = t <= 2 * Kr ? s_fr[t] : 0.0f;
        orr[g] = t <= 2 * Kr ? s_or[t] : 0;
        wa[g] = t <= 2 * Ka ? s_wa[t] : 0.0f;
    }

    // tile column tx of a bitmap starts, in its row i, at column 64 tx - smax + sh(i): the first one reaches column 0 in the row
    // that leans furthest, the last one column W - 1 in the row that leans least
    const int tiles_x = (W + (p.smax - p.smin) + kBlurTileCols - 1) / kBlurTileCols;
    const int tiles = tiles_x * ((Hh + TR - 1) / TR);
    // the tail lanes of the column pass: lane l < 8 owns column 64 + l % 4 of the round's row l / 4
    const int tail_row = lane < kBlurTailCols * kBlurRound ? lane / kBlurTailCols : 0;
    const int tail_col = lane < kBlurTailCols * kBlurRound ? kBlurTileCols + lane % kBlurTailCols : kBlurTileCols;

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int r0 = (tile / tiles_x) * TR;
        const int c0 = (tile % tiles_x) * kBlurTileCols - p.smax;
        {   // a tile none of whose rows meets the image (a corner of the leaning grid): nothing to write
            const int rows = min(TR, Hh - r0);
            const int a0 = c0 + blur_shear(p, 0), a1 = c0 + blur_shear(p, rows - 1);
            if (max(a0, a1) + kBlurTileCols <= 0 || min(a0, a1) >= W) continue;
        }

        // ---- column pass ----
        int nonzero = 0;
        float pre[kBlurRound][kBlurPrefetch];
        blur_fetch_rows(xb, p, r0, c0, kBlurRound * wave, rows_y, Hh, W, Wx, lane, pre);
        for (int jb = 0; jb < rows_y; jb += kBlurRound * kBlurWaves) {
            const int j = jb + kBlurRound * wave;
            int nz = 0;
#pragma unroll
            for (int q = 0; q < kBlurRound; ++q)
#pragma unroll
                for (int u = 0; u < kBlurPrefetch; ++u) {
                    const int i = lane + 64 * u;
                    if (i < Wx) strips[q * kBlurStrip + i] = pre[q][u];
                    nz |= (pre[q][u] != 0.0f);          // (a NaN is non-zero)
                }
            const int round_nonzero = __any(nz);
            if (lane == 0 && j < rows_y) s_live[j / kBlurRound] = round_nonzero;
            __syncthreads();
            if (jb + kBlurRound * kBlurWaves < rows_y)
                blur_fetch_rows(xb, p, r0, c0, j + kBlurRound * kBlurWaves, rows_y, Hh, W, Wx, lane, pre);
            if (j < rows_y) {
                float acc[kBlurRound], tail = 0.0f;
#pragma unroll
                for (int q = 0; q < kBlurRound; ++q) acc[q] = 0.0f;
                if (round_nonzero) {
                    nonzero = 1;
                    const float* __restrict__ xs = strips + lane;
                    const float* __restrict__ xt = strips + tail_row * kBlurStrip + tail_col;
#pragma unroll
                    for (int g = 0; g < 3; ++g)             // k = t - Ka ascending
                        blur_column_taps(acc, tail, wa[g], 64 * g, min(64 * g + 64, 2 * Ka + 1), Ka, xs, xt);
                }
#pragma unroll
                for (int q = 0; q < kBlurRound; ++q)
                    if (j + q < rows_y) Y[(j + q) * Wy + lane] = acc[q];
                if (lane < kBlurTailCols * kBlurRound && j + tail_row < rows_y) Y[(j + tail_row) * Wy + tail_col] = tail;
            }
            __syncthreads();        // (the strips are written again)
        }
        const int any_nonzero = __syncthreads_or(nonzero);
        // the rows of y that hold anything, j_lo .. j_hi - 1 (whole rounds): a tap into a row outside adds exactly +0
        int j_lo = rows_y, j_hi = 0;
        {
            const int rounds = (rows_y + kBlurRound - 1) / kBlurRound;
            constexpr int kWords = ((kBlurMaxTileRows + 2 * kBlurMaxRadius) / kBlurRound + 63) / 64;
#pragma unroll
            for (int u = kWords - 1; u >= 0; --u) {
                const int q = lane + 64 * u;
                const unsigned long long live = __ballot(q < rounds && s_live[q] != 0);
                if (live) j_lo = kBlurRound * (64 * u + __ffsll((long long)live) - 1);
            }
#pragma unroll
            for (int u = 0; u < kWords; ++u) {
                const int q = lane + 64 * u;
                const unsigned long long live = __ballot(q < rounds && s_live[q] != 0);
                if (live) j_hi = kBlurRound * (64 * u + 64 - __clzll((long long)live) + 0);
            }
            j_lo = __builtin_amdgcn_readfirstlane(j_lo);
            j_hi = __builtin_amdgcn_readfirstlane(j_hi);
        }

        // ---- sheared row pass ----
        // The tile's rows that meet the image are one run ia .. iz - 1 (the lean is monotone): blocks of 128 rows from ia, wave w
        // owns rows 8 w .. 8 w + 7 of a block.
        int ia, iz;
        {
            unsigned long long meets[kBlurMaxTileRows / 64];
#pragma unroll
            for (int u = 0; u < kBlurMaxTileRows / 64; ++u) {
                const int i = lane + 64 * u;
                const int first = c0 + blur_shear(p, i);
                meets[u] = __ballot(i < TR && r0 + i < Hh && first + kBlurTileCols > 0 && first < W);
            }
            ia = TR; iz = 0;
#pragma unroll
            for (int u = kBlurMaxTileRows / 64 - 1; u >= 0; --u)
                if (meets[u]) ia = 64 * u + __ffsll((long long)meets[u]) - 1;
#pragma unroll
            for (int u = 0; u < kBlurMaxTileRows / 64; ++u)
                if (meets[u]) iz = 64 * u + 64 - __clzll((long long)meets[u]);
            ia = __builtin_amdgcn_readfirstlane(ia);
            iz = __builtin_amdgcn_readfirstlane(iz);
        }
        for (int ib = ia; ib < iz; ib += kBlurWaves * kBlurRowsPerWave) {
            const int i0 = ib + kBlurRowsPerWave * wave;
            if (i0 >= iz) continue;         // (no barrier in this loop: a wave may leave it alone)
            float acc[kBlurRowsPerWave];
            int lane_term[kBlurRowsPerWave], row_of[kBlurRowsPerWave];
#pragma unroll
            for (int m = 0; m < kBlurRowsPerWave; ++m) {
                acc[m] = 0.0f;
                row_of[m] = min(i0 + m, iz - 1);
                lane_term[m] = 4 * (blur_shear(p, row_of[m]) + lane);
            }
            if (any_nonzero) {
                const bool clamped = i0 + kBlurRowsPerWave > iz;
                // row i reads row j = i + 2 Kr - t of y at tap t: the wave's taps that can meet a row with anything in it
                const int t_lo = max(0, i0 + 2 * Kr - (j_hi - 1));
                const int t_hi = min(2 * Kr, min(i0 + kBlurRowsPerWave, iz) - 1 + 2 * Kr - j_lo);
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    int t = max(64 * g, t_lo);
                    const int t1 = min(64 * g + 64, t_hi + 1);
                    if (clamped) {
                        blur_row_taps<kBlurRowsPerWave, true>(acc, lane_term, row_of, wr[g], fr[g], orr[g], 64 * g, t, t1, i0, Kr, s_row, Y);
                    } else {
                        for (; t + kBlurRowsPerWave <= t1; t += kBlurRowsPerWave)
                            blur_row_tap_block<kBlurRowsPerWave>(acc, lane_term, wr[g], fr[g], orr[g], 64 * g, t, i0, Kr, s_row, Y);
                        blur_row_taps<kBlurRowsPerWave, false>(acc, lane_term, row_of, wr[g], fr[g], orr[g], 64 * g, t, t1, i0, Kr, s_row, Y);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < kBlurRowsPerWave; ++m) {
                const int i = i0 + m;
                const int c = c0 + blur_shear(p, i) + lane;
                if (i < iz && c >= 0 && c < W) ob[(size_t)(r0 + i) * (size_t)W + c] = acc[m];
            }
        }
        __syncthreads();        // the next tile's column pass overwrites Y
    }
}

static LdsGrant g_blur_grant;

// The blur mode of art_flux_crop_fwd: covariance [B,3] = (Srr, Src, Scc) in pixels^2; x, out [B,Hh,W]; out fully written.
int flux_blur_launch(const float* x, const float* covariance, int64_t B, int64_t Hh, int64_t W, float* out, hipStream_t stream)
{
    if (B >= 0 && (B == 0 || Hh == 0 || W == 0) && Hh >= 0 && W >= 0) return ART_OK;
    if (!x || !covariance || !out || B < 0 || Hh < 1 || W < 1 || Hh > 65535 || W > 65535 * (int64_t)kBlurTileCols ||
        Hh * W > (int64_t)1 << 30 || B > 65535)
        return ART_EINVAL;
    const int64_t n = B * Hh * W;
    if (x < out + n && out < x + n) return ART_EINVAL;          // the row pass reads what another tile would have overwritten
    const size_t lds = (size_t)kBlurLdsFloats * sizeof(float);
    const int rc = grant_dynamic_lds(reinterpret_cast<const void*>(&flux_blur_kernel), g_blur_grant, lds);
    if (rc != ART_OK) return rc;
    // workgroups per bitmap: its tiles at a shear of half a column per row (more tiles - a steeper window - are walked in turns)
    const int64_t rows = (Hh + kBlurMaxTileRows - 1) / kBlurMaxTileRows;
    const int64_t lean = (Hh < kBlurMaxTileRows ? Hh : kBlurMaxTileRows) / 2;
    const int64_t groups = rows * ((W + lean + kBlurTileCols - 1) / kBlurTileCols);
    hipLaunchKernelGGL(flux_blur_kernel, dim3((unsigned)(groups < 65535 ? groups : 65535), (unsigned)B), dim3(kBlurBlock), lds, stream, x,
                       covariance, (int)Hh, (int)W, out);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

// ---- the gradient with respect to the window: the blur mode of art_flux_crop_bwd (include/artist_hip.h) ----------------------------
// Per bitmap, L = sum g z, z = blur(x; S) as above with the radii held fixed: three sums over the pixels,
//   D_v = sum g[r,c] sum_k w'(v)_k lerp(y [r - k, .], c - s k)         v = Srr
//   D_a = sum g[r,c] sum_k w (v)_k lerp(y'[r - k, .], c - s k)         y' = the column pass with w'(a)
//   D_s = sum g[r,c] sum_k w (v)_k (-k) d_k[r - k, c]                  d_k = the lerp's derivative with respect to its position
// w'_k = w_k (k^2 - m2) / (2 u^2), m2 = sum_j w_j j^2, and the chain rule to (Srr, Src, Scc) at the end.
//
// ONE workgroup per bitmap walks the forward's parallelogram tiles in ascending order, with at most 64 rows per tile: the images of
// y AND y' (each (64 + 128) x 68 floats) and the x strips are the forward's 129,792 B of LDS.  Column pass: the forward's, with a
// second accumulator for w'(a).  Row pass: wave w owns rows 4 w .. 4 w + 3 of the tile, lane l the column c0 + sh(i) + l; the
// three sums of a pixel are fp32 in ascending k, multiplied by g in fp32 and added to the lane's three fp64 sums - tiles in
// ascending order, rows in ascending order.  At the end a butterfly per wave, the waves' sums in ascending order by one thread,
// and the chain rule in fp64.  No atomics, no scratch, nothing read back: a bitmap's three values depend on its own x, g,
// covariance and (Hh, W) alone.
constexpr int kBlurGradTileRows = 64;
constexpr int kBlurGradRowsY = kBlurGradTileRows + 2 * kBlurMaxRadius;                 // 192 rows of y (and of y') per tile
constexpr int kBlurGradRowsPerWave = kBlurGradTileRows / kBlurWaves;                   // 4
constexpr int kBlurGradLdsFloats = 2 * kBlurGradRowsY * kBlurImageCols + kBlurWaves * kBlurRound * kBlurStrip;      // 129,792 B

// blur_weights and the derivative of every weight with respect to the variance, wd[0 .. 2K]: both from the fp64 weights.
__device__ __forceinline__ void blur_weights_grad(double v, int K, int lane, float* __restrict__ w, float* __restrict__ wd)
{
    const int k = lane + 1;
    const double e = k <= K ? exp(-(double)(k * k) / (2.0 * v)) : 0.0;
    double sum = e, moment = e * (double)(k * k);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        moment += __shfl_xor(moment, off, 64);
    }
    const double total = 1.0 + 2.0 * sum;
    const double m2 = 2.0 * moment / total;
    const double scale = K > 0 ? 1.0 / (2.0 * v * v) : 0.0;       // an identity pass does not depend on its variance
    if (lane == 0) {
        w[K] = (float)(1.0 / total);
        wd[K] = K > 0 ? (float)((1.0 / total) * (0.0 - m2) * scale) : 0.0f;
    }
    if (k <= K) {
        const double wk = e / total;
        const float d = (float)(wk * ((double)(k * k) - m2) * scale);
        w[K + k] = (float)wk;
        w[K - k] = (float)wk;
        wd[K + k] = d;
        wd[K - k] = d;
    }
}

// blur_column_taps for y and y' at once: the same x, the weights w(a) and w'(a).
__device__ __forceinline__ void blur_column_taps_grad(float (&acc)[kBlurRound], float (&dacc)[kBlurRound], float& tail, float& dtail,
                                                      float tw, float td, int t0, int t1, int Ka, const float* __restrict__ xs,
                                                      const float* __restrict__ xt)
{
    for (int t = t0; t < t1; ++t) {
        const float w = blur_lane_f(tw, t - t0);
        const float d = blur_lane_f(td, t - t0);
        const int q0 = 2 * Ka - t;
#pragma unroll
        for (int q = 0; q < kBlurRound; ++q) {
            const float xv = xs[q * kBlurStrip + q0];
            acc[q] = __builtin_fmaf(w, xv, acc[q]);
            dacc[q] = __builtin_fmaf(d, xv, dacc[q]);
        }
        const float xv = xt[q0];
        tail = __builtin_fmaf(w, xv, tail);
        dtail = __builtin_fmaf(d, xv, dtail);
    }
}

__global__ __launch_bounds__(kBlurBlock) void flux_blur_grad_kernel(const float* __restrict__ x, const float* __restrict__ cov,
                                                                    const float* __restrict__ g, int Hh, int W, float* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float blur_lds[];
    __shared__ float s_wr[kBlurTaps], s_dr[kBlurTaps], s_fr[kBlurTaps], s_wa[kBlurTaps], s_da[kBlurTaps];
    __shared__ int s_or[kBlurTaps];
    __shared__ int s_row[kBlurGradRowsY];                      // see blur_row_taps
    __shared__ int s_live[kBlurGradRowsY / kBlurRound];        // per round of the column pass: any input non-zero
    __shared__ double s_part[kBlurWaves][3];

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t image = (size_t)b * (size_t)Hh * (size_t)W;
    const float* __restrict__ xb = x + image;
    const float* __restrict__ gb = g + image;
    float* __restrict__ ob = out + 3 * (size_t)b;
    BlurPlan p = blur_plan(cov + 3 * (size_t)b, Hh);
    p.valid = __builtin_amdgcn_readfirstlane(p.valid);
    p.Kr = __builtin_amdgcn_readfirstlane(p.Kr);
    p.Ka = __builtin_amdgcn_readfirstlane(p.Ka);
    p.TR = __builtin_amdgcn_readfirstlane(p.TR);
    p.sfix = __builtin_amdgcn_readfirstlane(p.sfix);
    p.sbits = __builtin_amdgcn_readfirstlane(p.sbits);

    if (!p.valid) {         // the forward marks this bitmap NaN: so is its gradient
        if (tid < 3) ob[tid] = __builtin_nanf("");
        return;
    }
    {   // the forward's tiling at no more than 64 rows: two images of y fit where the forward keeps one
        p.TR = min(p.TR, kBlurGradTileRows);
        const int last = (p.sfix * (p.TR - 1)) >> p.sbits;
        p.smin = min(0, last);
        p.smax = max(0, last);
    }

    const int Kr = p.Kr, Ka = p.Ka, TR = p.TR;
    constexpr int Wy = kBlurImageCols;
    constexpr int kImageBytes = kBlurGradRowsY * Wy * (int)sizeof(float);
    const int rows_y = TR + 2 * Kr;
    const int Wx = Wy + 2 * Ka;
    float* __restrict__ Y = blur_lds;                                                   // [rows_y][Wy]
    float* __restrict__ Yd = blur_lds + kBlurGradRowsY * Wy;                            // y', the same layout
    float* __restrict__ strips = blur_lds + 2 * kBlurGradRowsY * Wy + wave * kBlurRound * kBlurStrip;

    if (wave == 0) blur_weights_grad(p.Srr, Kr, lane, s_wr, s_dr);
    if (wave == 1) blur_weights_grad(p.a, Ka, lane, s_wa, s_da);
    if (tid >= 128 && tid < 128 + 2 * Kr + 1) {
        const int k = tid - 128 - Kr;
        const double pos = -p.s * (double)k;
        const double fl = floor(pos);
        s_or[tid - 128] = (int)fl;
        s_fr[tid - 128] = (float)(pos - fl);
    }
    for (int j = tid; j < kBlurGradRowsY; j += kBlurBlock) s_row[j] = 4 * (j * Wy - blur_shear(p, j - Kr) + 2);
    __syncthreads();
    float wr[3], dr[3], fr[3], wa[3], da[3];
    int orr[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int t = lane + 64 * q;
        wr[q] = t <= 2 * Kr ? s_wr[t] : 0.0f;
        dr[q] = t <= 2 * Kr ? s_dr[t] : 0.0f;
        fr[q] = t <= 2 * Kr ? s_fr[t] : 0.0f;
        orr[q] = t <= 2 * Kr ? s_or[t] : 0;
        wa[q] = t <= 2 * Ka ? s_wa[t] : 0.0f;
        da[q] = t <= 2 * Ka ? s_da[t] : 0.0f;
    }

    const int tiles_x = (W + (p.smax - p.smin) + kBlurTileCols - 1) / kBlurTileCols;
    const int tiles = tiles_x * ((Hh + TR - 1) / TR);
    const int tail_row = lane < kBlurTailCols * kBlurRound ? lane / kBlurTailCols : 0;
    const int tail_col = lane < kBlurTailCols * kBlurRound ? kBlurTileCols + lane % kBlurTailCols : kBlurTileCols;

    double sum_v = 0.0, sum_a = 0.0, sum_s = 0.0;          // this lane's pixels, tiles and rows in ascending order

    for (int tile = 0; tile < tiles; ++tile) {
        const int r0 = (tile / tiles_x) * TR;
        const int c0 = (tile % tiles_x) * kBlurTileCols - p.smax;
        {   // a corner of the leaning grid
            const int rows = min(TR, Hh - r0);
            const int a0 = c0 + blur_shear(p, 0), a1 = c0 + blur_shear(p, rows - 1);
            if (max(a0, a1) + kBlurTileCols <= 0 || min(a0, a1) >= W) continue;
        }

        // ---- column pass: y and y' ----
        int nonzero = 0;
        float pre[kBlurRound][kBlurPrefetch];
        blur_fetch_rows(xb, p, r0, c0, kBlurRound * wave, rows_y, Hh, W, Wx, lane, pre);
        for (int jb = 0; jb < rows_y; jb += kBlurRound * kBlurWaves) {
            const int j = jb + kBlurRound * wave;
            int nz = 0;
#pragma unroll
            for (int q = 0; q < kBlurRound; ++q)
#pragma unroll
                for (int u = 0; u < kBlurPrefetch; ++u) {
                    const int i = lane + 64 * u;
                    if (i < Wx) strips[q * kBlurStrip + i] = pre[q][u];
                    nz |= (pre[q][u] != 0.0f);
                }
            const int round_nonzero = __any(nz);
            if (lane == 0 && j < rows_y) s_live[j / kBlurRound] = round_nonzero;
            __syncthreads();
            if (jb + kBlurRound * kBlurWaves < rows_y)
                blur_fetch_rows(xb, p, r0, c0, j + kBlurRound * kBlurWaves, rows_y, Hh, W, Wx, lane, pre);
            if (j < rows_y) {
                float acc[kBlurRound], dacc[kBlurRound], tail = 0.0f, dtail = 0.0f;
#pragma unroll
                for (int q = 0; q < kBlurRound; ++q) acc[q] = dacc[q] = 0.0f;
                if (round_nonzero) {
                    nonzero = 1;
                    const float* __restrict__ xs = strips + lane;
                    const float* __restrict__ xt = strips + tail_row * kBlurStrip + tail_col;
#pragma unroll
                    for (int q = 0; q < 3; ++q)             // k = t - Ka ascending
                        blur_column_taps_grad(acc, dacc, tail, dtail, wa[q], da[q], 64 * q, min(64 * q + 64, 2 * Ka + 1), Ka, xs, xt);
                }
#pragma unroll
                for (int q = 0; q < kBlurRound; ++q)
                    if (j + q < rows_y) {
                        Y[(j + q) * Wy + lane] = acc[q];
                        Yd[(j + q) * Wy + lane] = dacc[q];
                    }
                if (lane < kBlurTailCols * kBlurRound && j + tail_row < rows_y) {
                    Y[(j + tail_row) * Wy + tail_col] = tail;
                    Yd[(j + tail_row) * Wy + tail_col] = dtail;
                }
            }
            __syncthreads();        // (the strips are written again)
        }
        const int any_nonzero = __syncthreads_or(nonzero);
        // the rows of y that hold anything, j_lo .. j_hi - 1 (whole rounds): a tap into a row outside adds exactly 0
        int j_lo = rows_y, j_hi = 0;
        {
            const int rounds = (rows_y + kBlurRound - 1) / kBlurRound;
            constexpr int kWords = (kBlurGradRowsY / kBlurRound + 63) / 64;
#pragma unroll
            for (int u = kWords - 1; u >= 0; --u) {
                const int q = lane + 64 * u;
                const unsigned long long live = __ballot(q < rounds && s_live[q] != 0);
                if (live) j_lo = kBlurRound * (64 * u + __ffsll((long long)live) - 1);
            }
#pragma unroll
            for (int u = 0; u < kWords; ++u) {
                const int q = lane + 64 * u;
                const unsigned long long live = __ballot(q < rounds && s_live[q] != 0);
                if (live) j_hi = kBlurRound * (64 * u + 64 - __clzll((long long)live));
            }
            j_lo = __builtin_amdgcn_readfirstlane(j_lo);
            j_hi = __builtin_amdgcn_readfirstlane(j_hi);
        }

        // ---- the three sheared row passes ----
        int ia = TR, iz = 0;
        {
            const int first = c0 + blur_shear(p, lane);
            const unsigned long long meets = __ballot(lane < TR && r0 + lane < Hh && first + kBlurTileCols > 0 && first < W);
            if (meets) {
                ia = __ffsll((long long)meets) - 1;
                iz = 64 - __clzll((long long)meets);
            }
            ia = __builtin_amdgcn_readfirstlane(ia);
            iz = __builtin_amdgcn_readfirstlane(iz);
        }
        const int i0 = ia + kBlurGradRowsPerWave * wave;
        if (any_nonzero && i0 < iz) {
            float acc_v[kBlurGradRowsPerWave], acc_a[kBlurGradRowsPerWave], acc_s[kBlurGradRowsPerWave], gv[kBlurGradRowsPerWave];
            int lane_term[kBlurGradRowsPerWave], row_of[kBlurGradRowsPerWave];
#pragma unroll
            for (int m = 0; m < kBlurGradRowsPerWave; ++m) {
                acc_v[m] = acc_a[m] = acc_s[m] = 0.0f;
                row_of[m] = min(i0 + m, iz - 1);             // rows past the run's end repeat its last row and are not summed
                const int lean = blur_shear(p, row_of[m]);
                lane_term[m] = 4 * (lean + lane);
                const int c = c0 + lean + lane;
                const bool inside = i0 + m < iz && c >= 0 && c < W;
                gv[m] = inside ? gb[(size_t)(r0 + row_of[m]) * (size_t)W + c] : 0.0f;
            }
            // row i reads row j = i + 2 Kr - t of y at tap t: the wave's taps that can meet a row with anything in it
            const int t_lo = max(0, i0 + 2 * Kr - (j_hi - 1));
            const int t_hi = min(2 * Kr, min(i0 + kBlurGradRowsPerWave, iz) - 1 + 2 * Kr - j_lo);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int t1 = min(64 * q + 64, t_hi + 1);
                for (int t = max(64 * q, t_lo); t < t1; ++t) {
                    const float w = blur_lane_f(wr[q], t - 64 * q);
                    const float d = blur_lane_f(dr[q], t - 64 * q);
                    const float f = blur_lane_f(fr[q], t - 64 * q);
                    const int o4 = 4 * __builtin_amdgcn_readlane(orr[q], t - 64 * q);
                    const float wk = w * (float)(Kr - t);             // w_k (-k)
                    const bool whole = f == 0.0f;                     // -s k is an integer: the mean of the two one-sided slopes
#pragma unroll
                    for (int m = 0; m < kBlurGradRowsPerWave; ++m) {
                        const int row = s_row[row_of[m] + 2 * Kr - t];
                        const char* at = reinterpret_cast<const char*>(Y) + (row + lane_term[m] + o4);
                        const float* __restrict__ yr = reinterpret_cast<const float*>(at);
                        const float* __restrict__ ur = reinterpret_cast<const float*>(at + kImageBytes);
                        const float v0 = yr[0], v1 = yr[1], u0 = ur[0], u1 = ur[1];
                        acc_v[m] = __builtin_fmaf(d, __builtin_fmaf(f, v1 - v0, v0), acc_v[m]);
                        acc_a[m] = __builtin_fmaf(w, __builtin_fmaf(f, u1 - u0, u0), acc_a[m]);
                        const float slope = whole ? 0.5f * (v1 - yr[-1]) : v1 - v0;
                        acc_s[m] = __builtin_fmaf(wk, slope, acc_s[m]);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < kBlurGradRowsPerWave; ++m) {
                const int c = c0 + blur_shear(p, row_of[m]) + lane;
                if (i0 + m < iz && c >= 0 && c < W) {
                    sum_v += (double)(gv[m] * acc_v[m]);
                    sum_a += (double)(gv[m] * acc_a[m]);
                    sum_s += (double)(gv[m] * acc_s[m]);
                }
            }
        }
        __syncthreads();        // the next tile's column pass overwrites y and y'
    }

    // the lanes of a wave (a butterfly: the same order in every run), then the waves in ascending order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum_v += __shfl_xor(sum_v, off, 64);
        sum_a += __shfl_xor(sum_a, off, 64);
        sum_s += __shfl_xor(sum_s, off, 64);
    }
    if (lane == 0) {
        s_part[wave][0] = sum_v;
        s_part[wave][1] = sum_a;
        s_part[wave][2] = sum_s;
    }
    __syncthreads();
    if (tid == 0) {
        double Dv = 0.0, Da = 0.0, Ds = 0.0;
        for (int q = 0; q < kBlurWaves; ++q) {
            Dv += s_part[q][0];
            Da += s_part[q][1];
            Ds += s_part[q][2];
        }
        if (Kr == 0) {          // the row pass is the identity: a = Scc
            ob[0] = 0.0f;
            ob[1] = 0.0f;
            ob[2] = (float)Da;
        } else {
            const double v = p.Srr, s = p.s;
            ob[0] = (float)(Dv - (s / v) * Ds + s * s * Da);
            ob[1] = (float)(Ds / v - 2.0 * s * Da);
            ob[2] = (float)Da;
        }
    }
}

static LdsGrant g_blur_grad_grant;

// The blur mode of art_flux_crop_bwd: x, g [B,Hh,W], covariance [B,3]; out [B,3] = dL/d(Srr, Src, Scc), fully written.
int flux_blur_grad_launch(const float* x, const float* covariance, const float* g, int64_t B, int64_t Hh, int64_t W, float* out,
                          hipStream_t stream)
{
    if (B >= 0 && (B == 0 || Hh == 0 || W == 0) && Hh >= 0 && W >= 0) return ART_OK;
    if (!x || !covariance || !g || !out || B < 0 || Hh < 1 || W < 1 || Hh > 65535 || W > 65535 * (int64_t)kBlurTileCols ||
        Hh * W > (int64_t)1 << 30 || B > 65535)
        return ART_EINVAL;
    const int64_t n = B * Hh * W;
    if ((x < out + 3 * B && out < x + n) || (g < out + 3 * B && out < g + n) || (covariance < out + 3 * B && out < covariance + 3 * B))
        return ART_EINVAL;
    const size_t lds = (size_t)kBlurGradLdsFloats * sizeof(float);
    const int rc = grant_dynamic_lds(reinterpret_cast<const void*>(&flux_blur_grad_kernel), g_blur_grad_grant, lds);
    if (rc != ART_OK) return rc;
    hipLaunchKernelGGL(flux_blur_grad_kernel, dim3((unsigned)B), dim3(kBlurBlock), lds, stream, x, covariance, g, (int)Hh, (int)W, out);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

}  // namespace art
