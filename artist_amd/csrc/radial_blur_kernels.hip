// radial_blur_kernels.hip - the convolved sun for radial shapes: one elliptical, non-separable window per bitmap (gfx950).
//
// The radial window mode of art_flux_crop_fwd (include/artist_hip.h, where the operator is defined).  Per bitmap b with metric
// M = (M_rr, M_rc, M_cc) in px^2/rad^2 and the sun's quantile table t2[0..K] in rad^2: the stencil w[dr, dc] is the 4 x 4 sub-pixel
// mean of the table's density at q(dr, dc) = (dr, dc) M^-1 (dr, dc)^T, cut at the largest node k* whose ellipse fits 64 pixels and
// normalised to k* / K; z[r, c] = sum over dr, then dc, ascending, of fma(w[dr, dc], x[r - dr, c - dc], acc).  x is zero outside
// the image and z is cut to it; the stencil is point-symmetric, so the operator is its own adjoint.
//
// One kernel, no workspace, one workgroup per CU.  LDS holds the table, the stencil's rows dr >= 0 (row -dr is row dr read
// backwards) and one input tile with its halo.  A wave owns 64 output rows x 8 columns: lane l row l, its 8 columns in registers.
// For a stencil row and 8 of its taps the lane reads the 15 inputs x[r - dr, c0 - d0 - 7 ..] that its 8 x 8 (column, tap) pairs
// share, as 4 aligned 16-byte reads; the 8 weights come out of a register that holds 64 taps of the row, one per lane (readlane).
// Lanes one row apart read 4 x an odd number of floats apart: no bank conflict.  Only each stencil row's span of non-zero taps is walked,
// in blocks of 8 (a zero tap in a block adds w * x = 0: the same bits for a finite x), and only the taps that can meet the box around the
// tile's non-zero inputs; a tile whose inputs are all zero is written as zeros, and the stencil is built when a workgroup meets its
// first tile that is not.  The tiling depends on the bitmap's own metric, the table and (Hh, W) alone, and an output's sum on
// neither: a bitmap's bits depend neither on B, nor on its place in the batch, nor on the run.  No float atomics.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "launch_common.hpp"

namespace art {

constexpr int kRadBlock = 1024;                 // 16 waves: one workgroup per CU (the LDS image), 4 waves per SIMD
constexpr int kRadWaves = kRadBlock / 64;
constexpr int kRadMaxRadius = 64;               // taps -64..64 in rows and columns: the blur mode's own limit
constexpr int kRadMaxK = 4096;
constexpr int kRadCols = 8;                     // output columns per lane
constexpr int kRadReads = 2 * kRadCols;         // inputs that 8 columns x 8 taps share: 15, read as 4 x 4
constexpr int kRadRowLoads = 4;                 // a tile row is at most radial_stride(64 + 2 * 64 + 7) = 204 <= 256 floats: 4 per lane
constexpr int kRadLdsFloats = 38912;            // 152 KiB of dynamic LDS: table, half stencil, tile
constexpr int kRadMaxTapsPerThread = ((kRadMaxRadius + 1) * (2 * kRadMaxRadius + 1) + kRadBlock - 1) / kRadBlock;       // 9
constexpr double kRadLimit2 = (double)(kRadMaxRadius * kRadMaxRadius);
constexpr double kRadMinDet = 1e-6;             // det <= 1e-6 M_rr M_cc: the metric is rank-deficient, the bitmap NaN

// How a tile is laid over the waves: WR x WC waves of RW rows x 8 columns.  The first shape whose tile and halo fit beside the
// table and the stencil is taken; the last one fits at K = 4096 and both radii 64: (32 + 128) x 143 + 4100 + 8388 <= 38912.
struct RadialShape { int WR, WC, RW; };
__device__ static constexpr RadialShape kRadShapes[6] = {{2, 8, 64}, {1, 8, 64}, {1, 4, 64}, {1, 2, 64}, {1, 1, 64}, {1, 1, 32}};

// Floats per tile row of `cols` columns: four more (a block of taps may start up to three taps early and reads 16 inputs for its
// 15), then up to the next 4 (mod 8) - every row starts 16-byte aligned, and the 16-byte reads of 16 lanes one row apart (4 x an
// odd number of floats) fall on 16 different quads of the LDS's 64 banks.
__device__ __forceinline__ constexpr int radial_stride(int cols)
{
    const int s = cols + 4;
    return s + ((12 - (s & 7)) & 7);
}

// The density of the table at q: 1 / (t2[k+1] - t2[k]) for the largest k with t2[k] <= q, 0 unless 0 <= k < kstar.
__device__ __forceinline__ double radial_density(const float* __restrict__ tb, int kstar, double q)
{
    int lo = 0, hi = kstar + 1;         // the number of entries t2[0..kstar] that are <= q
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((double)tb[mid] <= q) lo = mid + 1; else hi = mid;
    }
    const int k = lo - 1;
    if (k < 0 || k >= kstar) return 0.0;
    return 1.0 / ((double)tb[k + 1] - (double)tb[k]);
}

__global__ __launch_bounds__(kRadBlock) void flux_radial_blur_kernel(const float* __restrict__ x, const float* __restrict__ metric,
                                                                      const float* __restrict__ table, int K, int Hh, int W,
                                                                      float* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float rad_lds[];
    __shared__ double s_sum[kRadWaves];
    __shared__ int s_lo[kRadMaxRadius + 1], s_hi[kRadMaxRadius + 1];      // per stencil row dr >= 0: its first and last non-zero tap
    __shared__ int s_box[4];                                               // the tile's non-zero inputs: rows lo, hi, columns lo, hi

    const int b = blockIdx.y;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t image = (size_t)b * (size_t)Hh * (size_t)W;
    const float* __restrict__ xb = x + image;
    float* __restrict__ ob = out + image;

    // ---- the metric, the table into LDS, k* ----
    const double Mrr = (double)metric[3 * (size_t)b], Mrc = (double)metric[3 * (size_t)b + 1], Mcc = (double)metric[3 * (size_t)b + 2];
    const double det = Mrr * Mcc - Mrc * Mrc;
    const bool metric_ok = isfinite(Mrr) && isfinite(Mrc) && isfinite(Mcc) && Mrr > 0.0 && Mcc > 0.0 && det > kRadMinDet * (Mrr * Mcc);
    float* __restrict__ tb = rad_lds;                                      // [K + 1]
    int table_bad = 0, fitting = 0;
    for (int base = 0; base <= K; base += kRadBlock) {
        const int k = base + tid;
        const bool in = k <= K;
        const float v = in ? table[k] : 0.0f;
        if (in) {
            tb[k] = v;
            table_bad |= !isfinite(v) || (k == 0 ? v < 0.0f : v < table[k - 1]);
        }
        // node k fits: both half extents sqrt(t2[k] M) <= 64 (the products of two floats are exact in fp64)
        const bool fits = in && metric_ok && (double)v * Mrr <= kRadLimit2 && (double)v * Mcc <= kRadLimit2;
        fitting += __syncthreads_count(fits);
    }
    table_bad = __syncthreads_or(table_bad);
    const int kstar = __builtin_amdgcn_readfirstlane(fitting) - 1;         // (the table does not decrease: the nodes that fit are a prefix)

    if (table_bad || !metric_ok || kstar < 1) {         // marked in the result itself: the whole bitmap is NaN
        const size_t n = (size_t)Hh * (size_t)W;
        for (size_t i = (size_t)blockIdx.x * kRadBlock + tid; i < n; i += (size_t)gridDim.x * kRadBlock) ob[i] = __builtin_nanf("");
        return;
    }

    // ---- the stencil's box and the tile's shape ----
    const double T = (double)tb[kstar];
    const int Rr = __builtin_amdgcn_readfirstlane(min(kRadMaxRadius, (int)floor(sqrt(T * Mrr) + 0.375)));
    const int Rc = __builtin_amdgcn_readfirstlane(min(kRadMaxRadius, (int)floor(sqrt(T * Mcc) + 0.375)));
    const int Ws = 2 * Rc + 1;
    const int table_floats = (K + 1 + 3) & ~3;
    const int stencil_floats = ((Rr + 1) * Ws + 3) & ~3;
    float* __restrict__ st = rad_lds + table_floats;                       // [Rr + 1][Ws]: rows dr = 0..Rr, columns -Rc..Rc
    float* __restrict__ tile = st + stencil_floats;
    const int Wt_halo = 2 * Rc + kRadCols - 1;                             // tile columns beside its own: Rc + 7 to the left, Rc to the right
    int WR = 1, WC = 1, RW = 32;
#pragma unroll
    for (int s = 5; s >= 0; --s) {
        const RadialShape shape = kRadShapes[s];
        const int rows = shape.WR * shape.RW + 2 * Rr, stride = radial_stride(shape.WC * kRadCols + Wt_halo);
        if (rows * stride <= kRadLdsFloats - table_floats - stencil_floats) { WR = shape.WR; WC = shape.WC; RW = shape.RW; }
    }
    const int TR = WR * RW, TC = WC * kRadCols;
    const int Wt = TC + Wt_halo;
    const int stride = radial_stride(Wt);
    const float4* __restrict__ tile4 = reinterpret_cast<const float4*>(tile);
    const int rows_t = TR + 2 * Rr;
    const int tiles_x = (W + TC - 1) / TC;
    const int tiles = tiles_x * ((Hh + TR - 1) / TR);
    const int wr = wave / WC, wc = wave - wr * WC;
    const bool wave_active = wave < WR * WC;
    const int lrow = min(lane, RW - 1);         // (RW = 32: the upper half of the wave repeats row 31 and stores nothing)
    int built = 0;

    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int r0 = (t / tiles_x) * TR;
        const int c0 = (t % tiles_x) * TC;
        const int row_base = r0 - Rr, col_base = c0 - Rc - (kRadCols - 1);  // the image coordinates of the tile's element (0, 0)
        if (tid == 0) { s_box[0] = INT_MAX; s_box[1] = INT_MIN; s_box[2] = INT_MAX; s_box[3] = INT_MIN; }
        __syncthreads();

        // ---- the tile and its halo, zero outside the image; the box around what is not zero ----
        int rlo = INT_MAX, rhi = INT_MIN, clo = INT_MAX, chi = INT_MIN;
#pragma unroll 2
        for (int i = wave; i < rows_t; i += kRadWaves) {
            const int r = row_base + i;
            const bool live = r >= 0 && r < Hh;
            const float* __restrict__ xr = xb + (size_t)(live ? r : 0) * (size_t)W;
            float pre[kRadRowLoads];            // (a row's loads are in flight together)
#pragma unroll
            for (int u = 0; u < kRadRowLoads; ++u) {
                const int j = lane + 64 * u, c = col_base + j;
                pre[u] = (live && j < Wt && c >= 0 && c < W) ? xr[c] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < kRadRowLoads; ++u) {
                const int j = lane + 64 * u, c = col_base + j;
                if (j < stride) tile[i * stride + j] = pre[u];
                if (pre[u] != 0.0f) {       // (a NaN is non-zero)
                    rlo = min(rlo, r); rhi = max(rhi, r);
                    clo = min(clo, c); chi = max(chi, c);
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            rlo = min(rlo, __shfl_xor(rlo, off, 64)); rhi = max(rhi, __shfl_xor(rhi, off, 64));
            clo = min(clo, __shfl_xor(clo, off, 64)); chi = max(chi, __shfl_xor(chi, off, 64));
        }
        if (lane == 0 && rlo <= rhi) {
            atomicMin(&s_box[0], rlo); atomicMax(&s_box[1], rhi);
            atomicMin(&s_box[2], clo); atomicMax(&s_box[3], chi);
        }
        __syncthreads();
        const int box_rlo = __builtin_amdgcn_readfirstlane(s_box[0]), box_rhi = __builtin_amdgcn_readfirstlane(s_box[1]);
        const int box_clo = __builtin_amdgcn_readfirstlane(s_box[2]), box_chi = __builtin_amdgcn_readfirstlane(s_box[3]);

        if (box_rlo > box_rhi) {            // nothing but zeros under this tile's window
            const int rows = min(TR, Hh - r0), cols = min(TC, W - c0);
            for (int i = tid; i < rows * cols; i += kRadBlock) ob[(size_t)(r0 + i / cols) * (size_t)W + c0 + i % cols] = 0.0f;
            __syncthreads();                // (the next tile writes s_box)
            continue;
        }

        if (!built) {
            // ---- the stencil: rows dr = 0..Rr, every weight formed in fp64 and rounded once ----
            built = 1;
            const int ntaps = (Rr + 1) * Ws;
            double raws[kRadMaxTapsPerThread];
            double part = 0.0;
#pragma unroll
            for (int n = 0; n < kRadMaxTapsPerThread; ++n) {
                const int tap = tid + n * kRadBlock;
                double raw = 0.0;
                if (tap < ntaps) {
                    const int dr = tap / Ws, dc = tap - dr * Ws - Rc;
                    double sum = 0.0;
                    // eight pairs of opposite sub-pixel points, (i, j) and (3 - i, 3 - j): the tap (-dr, -dc) sums the same pairs in
                    // the same order, so the stencil is point-symmetric to the bit
#pragma unroll 1
                    for (int p = 0; p < 8; ++p) {
                        double rho[2];
#pragma unroll
                        for (int side = 0; side < 2; ++side) {
                            const int i = side ? 3 - (p >> 2) : p >> 2, j = side ? 3 - (p & 3) : p & 3;
                            const double pr = (double)dr + (double)(2 * i - 3) * 0.125, pc = (double)dc + (double)(2 * j - 3) * 0.125;
                            const double q = (((Mcc * pr) * pr - ((2.0 * Mrc) * pr) * pc) + (Mrr * pc) * pc) / det;
                            rho[side] = radial_density(tb, kstar, q);
                        }
                        sum += rho[0] + rho[1];
                    }
                    raw = sum * 0.0625;
                    part += dr == 0 ? raw : 2.0 * raw;          // row -dr holds the same weights
                }
                raws[n] = raw;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
            if (lane == 0) s_sum[wave] = part;
            __syncthreads();
            double total = 0.0;
#pragma unroll
            for (int w = 0; w < kRadWaves; ++w) total += s_sum[w];
            const double kept = (double)kstar / (double)K;
#pragma unroll
            for (int n = 0; n < kRadMaxTapsPerThread; ++n) {
                const int tap = tid + n * kRadBlock;
                if (tap < ntaps) {
                    // far below a pixel, or a table of zeros: the one tap (0, 0) of weight k* / K
                    st[tap] = total > 0.0 ? (float)(raws[n] * kept / total) : (tap == Rc ? (float)kept : 0.0f);
                }
            }
            __syncthreads();
            if (tid <= Rr) {
                int lo = 1, hi = 0;
                for (int j = 0; j < Ws; ++j)
                    if (st[tid * Ws + j] != 0.0f) { if (lo > hi) lo = j - Rc; hi = j - Rc; }
                s_lo[tid] = lo; s_hi[tid] = hi;
            }
            __syncthreads();
        }

        // ---- the convolution: wave (wr, wc) owns rows r0w + l and columns cw .. cw + 7 ----
        const int r0w = r0 + wr * RW, cw = c0 + wc * kRadCols;
        if (wave_active && r0w < Hh && cw < W) {
            float acc[kRadCols];
#pragma unroll
            for (int j = 0; j < kRadCols; ++j) acc[j] = 0.0f;
            // row r reads row r - dr, column c column c - dc: the taps that can meet the box of non-zero inputs
            const int dr_lo = max(-Rr, r0w - box_rhi), dr_hi = min(Rr, r0w + RW - 1 - box_rlo);
            const int dc_lo = cw - box_chi, dc_hi = cw + kRadCols - 1 - box_clo;
            // the lane's row of the tile at the column that tap 0 of a block of 8 reads for column cw - 7 (in floats; an even number)
            const int xl = (wr * RW + lrow + Rr) * stride + (cw - col_base) - (kRadCols - 1);
            // the spans of the stencil's rows 0..63, one per lane (row 64 stays in LDS)
            const int lo_v = s_lo[min(lane, Rr)], hi_v = s_hi[min(lane, Rr)];
            for (int dr = dr_lo; dr <= dr_hi; ++dr) {
                const int ar = dr < 0 ? -dr : dr;
                const int span_lo = ar < 64 ? __builtin_amdgcn_readlane(lo_v, ar) : __builtin_amdgcn_readfirstlane(s_lo[kRadMaxRadius]);
                const int span_hi = ar < 64 ? __builtin_amdgcn_readlane(hi_v, ar) : __builtin_amdgcn_readfirstlane(s_hi[kRadMaxRadius]);
                const int lo = dr < 0 ? -span_hi : span_lo, hi = dr < 0 ? -span_lo : span_hi;
                int first = max(lo, dc_lo);
                const int last = min(hi, dc_hi);
                // a block starts at a tap that is Rc (mod 4), so that its inputs start on a 16-byte boundary of the row: up to three
                // taps early - a tap outside the row's span has weight 0, one inside it meets inputs that are all zero
                first -= (first - Rc) & 3;
                const float* __restrict__ wrow = st + ar * Ws + Rc;          // tap dc of row dr: wrow[dc], of row -dr: wrow[-dc]
                const int xrow = xl - dr * stride;
                for (int cb = first; cb <= last; cb += 64) {
                    const int dcl = cb + lane;
                    // (before the span, past it: zero taps that fill the first and the last block)
                    const float wv = dcl <= last && dcl >= -Rc ? wrow[dr < 0 ? -dcl : dcl] : 0.0f;
                    const int taps = min(last - cb + 1, 64);
                    for (int o = 0; o < taps; o += kRadCols) {
                        // column cw + j at tap cb + o + u reads column cw + j - cb - o - u: entry j - u + 7 of these 15 (and one more)
                        const float4* __restrict__ xp = tile4 + ((xrow - (cb + o)) >> 2);
                        float xv[kRadReads];
#pragma unroll
                        for (int q = 0; q < kRadReads / 4; ++q) {
                            const float4 quad = xp[q];
                            xv[4 * q] = quad.x;
                            xv[4 * q + 1] = quad.y;
                            xv[4 * q + 2] = quad.z;
                            xv[4 * q + 3] = quad.w;
                        }
                        // (the 16th input has no tap; kept alive, so that the last read stays one 16-byte read instead of a
                        //  12-byte one, which takes the LDS twice as long)
                        asm volatile("" ::"v"(xv[kRadReads - 1]));
#pragma unroll
                        for (int u = 0; u < kRadCols; ++u) {
                            const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv), o + u));
#pragma unroll
                            for (int j = 0; j < kRadCols; ++j) acc[j] = __builtin_fmaf(w, xv[j - u + kRadCols - 1], acc[j]);
                        }
                    }
                }
            }
            const int r = r0w + lane;
            if (lane < RW && r < Hh) {
#pragma unroll
                for (int j = 0; j < kRadCols; ++j)
                    if (cw + j < W) ob[(size_t)r * (size_t)W + cw + j] = acc[j];
            }
        }
        __syncthreads();        // the next tile overwrites the tile and s_box
    }
}

static LdsGrant g_radial_grant;

// The radial window mode of art_flux_crop_fwd: metric [B,3] = (M_rr, M_rc, M_cc) in px^2/rad^2, table [K+1] in rad^2; x, out
// [B,Hh,W]; out fully written.
int flux_radial_blur_launch(const float* x, const float* metric, const float* table, int64_t K, int64_t B, int64_t Hh, int64_t W,
                            float* out, hipStream_t stream)
{
    if (K < 1 || K > kRadMaxK) return ART_EINVAL;
    if (B >= 0 && (B == 0 || Hh == 0 || W == 0) && Hh >= 0 && W >= 0) return ART_OK;
    if (!x || !metric || !table || !out || B < 0 || Hh < 1 || W < 1 || Hh > 65535 || W > 65535 * (int64_t)64 ||
        Hh * W > (int64_t)1 << 30 || B > 65535)
        return ART_EINVAL;
    const int64_t n = B * Hh * W;
    if (x < out + n && out < x + n) return ART_EINVAL;          // a tile's halo would read what another tile has written
    if (table < out + n && out < table + K + 1) return ART_EINVAL;
    if (metric < out + n && out < metric + 3 * B) return ART_EINVAL;
    const size_t lds = (size_t)kRadLdsFloats * sizeof(float);
    const int rc = grant_dynamic_lds(reinterpret_cast<const void*>(&flux_radial_blur_kernel), g_radial_grant, lds);
    if (rc != ART_OK) return rc;
    // workgroups per bitmap: its tiles at the largest shape, but no more than fill the chip a few times over - a workgroup that
    // walks several tiles builds its stencil once
    const int64_t tiles = ((Hh + 127) / 128) * ((W + 63) / 64);
    const int64_t share = (2048 + B - 1) / B;
    const int64_t groups = tiles < share ? tiles : share;
    hipLaunchKernelGGL(flux_radial_blur_kernel, dim3((unsigned)(groups < 65535 ? groups : 65535), (unsigned)B), dim3(kRadBlock), lds,
                       stream, x, metric, table, (int)K, (int)Hh, (int)W, out);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

}  // namespace art
