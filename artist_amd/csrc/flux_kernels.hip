// flux_kernels.hip - the flux epilogue that runs on the ray tracer's bitmaps every optimisation epoch (gfx950).
//
//   crop   crop_flux_distributions_around_center (artist/flux/bitmap.py:121-246): centre of mass -> affine grid
//          -> bilinear grid_sample (align_corners=True, zeros padding), forward and backward.  The sampling grid is
//          an axis-aligned affine map, so the backward w.r.t. the bitmap is written as a GATHER (every input pixel
//          sums the few output pixels that sampled it): deterministic, no atomics - torch's grid_sample backward
//          scatters with atomics.
//   loss   PixelLoss / KLDivergenceLoss (artist/optim/loss.py:251-410) with the reduction over the two bitmap
//          dimensions, forward and backward, one workgroup per sample; and the four gain-free kinds of art_flux_loss (Jensen-Shannon,
//          shape pixel loss, total variation, cosine), which the reference does not have.
//
// All of it is HBM-bound elementwise / reduction work on [B,Hh,W] fp32: one read and one write of the bitmaps.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <mutex>
#include <vector>

#include "launch_common.hpp"
#include "flux_moments.hpp"

namespace art {

constexpr int kFluxBlock = 256;
constexpr int kReduceBlock = kMomentsBlock;     // per-bitmap reductions: one workgroup per bitmap, 16 waves to hide latency

struct CropMap {       // pixel j of the output samples input coordinate ix(j); same arithmetic in every kernel
    float sx, sy, xc, yc;
    int W, Hh;
    __device__ __forceinline__ float ix(int j) const { return (((sx * lin11(j, W) + xc) + 1.0f) / 2.0f) * (float)(W - 1); }
    __device__ __forceinline__ float iy(int i) const { return (((sy * lin11(i, Hh) + yc) + 1.0f) / 2.0f) * (float)(Hh - 1); }
};

__device__ __forceinline__ CropMap make_map(const float* __restrict__ dims, float xc, float yc, int b, int W, int Hh, float crop_w,
                                            float crop_h)
{
    CropMap m;
    m.sx = crop_w / fmaxf(dims[2 * b], 1e-8f);           // bitmap.py:218-225
    m.sy = crop_h / fmaxf(dims[2 * b + 1], 1e-8f);
    m.xc = xc; m.yc = yc;
    m.W = W; m.Hh = Hh;
    return m;
}

// com[b] = (x centre, y centre, sum + 1e-8) of bitmap b, one pass, sums in fp64: in normalised coordinates for the crop
// (bitmap.py:165-182), or - get_center_of_mass (bitmap.py:12-71), what FocalSpotLoss (artist/optim/loss.py:124-250) and the
// kinematics reconstructor's validation (kinematics_reconstructor.py:120) ask of the tracer's bitmaps - in PIXEL coordinates
// (e, u) = sum_j j f / (sum f + 1e-8).
template <typename Weights>
__global__ __launch_bounds__(kReduceBlock) void flux_com_kernel(const float* __restrict__ flux, int Hh, int W, float* __restrict__ com)
{
    __shared__ double s_red[16 * 3];
    const int b = blockIdx.x;
    double a[3];
    moment_sums<Weights>(flux + (int64_t)b * Hh * W, Hh, W, 0, Hh, s_red, a);
    if (threadIdx.x == 0) {
        float xc, yc, S;
        centre_from_sums(a[0], a[1], a[2], xc, yc, S);
        com[3 * b] = xc; com[3 * b + 1] = yc; com[3 * b + 2] = S;
    }
}

// ---------------------------------------------------------------------------------------------------
// The bilinear sample of one output pixel (align_corners=True, zeros padding), in two halves because the map is separable: a
// thread that stays in one column (the forward crop; the fused kernels when the workgroup size is a multiple of the bitmap
// width: pixel k = tid + n * blockDim has j = tid % W) forms the column half once, and the row half is wave-uniform there.
// ---------------------------------------------------------------------------------------------------
struct CropAxis { int p0; float t; bool a, b; };      // first tap, weight of the second, which of the two lie in the bitmap
__device__ __forceinline__ CropAxis crop_axis(float c, int n)
{
    CropAxis h;
    const float c0 = floorf(c);
    h.t = c - c0; h.p0 = (int)c0;
    h.a = h.p0 >= 0 && h.p0 < n; h.b = h.p0 + 1 >= 0 && h.p0 + 1 < n;
    return h;
}
__device__ __forceinline__ CropAxis crop_column(const CropMap& m, int j) { return crop_axis(m.ix(j), m.W); }
__device__ __forceinline__ CropAxis crop_row(const CropMap& m, int i) { return crop_axis(m.iy(i), m.Hh); }

// The sample of output pixel (i, column x): the sum of the present taps in this order (an absent tap adds nothing, not + 0), and
// in `v` the four values (0 where a tap is absent) with the two weights, for whoever needs the sample's gradient.
// `pixel(k)`: element k of the bitmap - from global memory, or from the rows a workgroup has staged in LDS.
// (The row half is formed here and not handed in: as a local of the caller's loop it made the compiler unroll the fused KL kernels
//  with a remainder loop - 63 and 68 registers instead of 41 and 45, the forward kernel one occupancy step down.)
struct CropTaps { float v00, v01, v10, v11, tx, ty; };
template <typename Pixel>
__device__ __forceinline__ float crop_sample_from(Pixel&& pixel, const CropMap& m, const CropAxis& x, int i, CropTaps& v)
{
    const CropAxis y = crop_row(m, i);
    const float ty = y.t;
    v.tx = x.t; v.ty = ty;
    v.v00 = y.a && x.a ? pixel(y.p0 * m.W + x.p0) : 0.0f; v.v01 = y.a && x.b ? pixel(y.p0 * m.W + x.p0 + 1) : 0.0f;
    v.v10 = y.b && x.a ? pixel((y.p0 + 1) * m.W + x.p0) : 0.0f; v.v11 = y.b && x.b ? pixel((y.p0 + 1) * m.W + x.p0 + 1) : 0.0f;
    float acc = 0.0f;
    if (y.a && x.a) acc += v.v00 * ((1.0f - x.t) * (1.0f - ty));
    if (y.a && x.b) acc += v.v01 * (x.t * (1.0f - ty));
    if (y.b && x.a) acc += v.v10 * ((1.0f - x.t) * ty);
    if (y.b && x.b) acc += v.v11 * (x.t * ty);
    return acc;
}
__device__ __forceinline__ float crop_sample(const float* __restrict__ f, const CropMap& m, const CropAxis& x, int i, CropTaps& v)
{
    return crop_sample_from([&](int k) { return f[k]; }, m, x, i, v);
}

// d sample / d (ix, iy): grid_sample's gradient w.r.t. its grid, per pixel ...
__device__ __forceinline__ void crop_sample_gradient(const CropTaps& v, float& gx, float& gy)
{
    gx = (v.v01 - v.v00) * (1.0f - v.ty) + (v.v11 - v.v10) * v.ty;
    gy = (v.v10 - v.v00) * (1.0f - v.tx) + (v.v11 - v.v01) * v.tx;
}
// ... and, summed over a bitmap, through affine_grid's translation: the gradient of the two centre coordinates
__device__ __forceinline__ void finish_centre_gradient(double gx, double gy, int W, int Hh, float* __restrict__ g2)
{
    g2[0] = (float)(gx * (double)((float)(W - 1) / 2.0f));
    g2[1] = (float)(gy * (double)((float)(Hh - 1) / 2.0f));
}

// grid (ceil(W / 256), ceil(Hh / kCropRows), B): a thread walks kCropRows output pixels of one column (the column's
// sampling coordinate and weights are computed once; a row's are wave-uniform).  One row per workgroup was 256 000
// workgroups of one pixel per thread for the metric field - dispatch and map set-up dominated (0.30 ms for 0.13 ms of
// HBM traffic).
constexpr int kCropRows = 8;
__global__ __launch_bounds__(kFluxBlock) void flux_crop_fwd_kernel(const float* __restrict__ flux,
                                                                   const float* __restrict__ dims,
                                                                   const float* __restrict__ com, int Hh, int W,
                                                                   float crop_w, float crop_h, float* __restrict__ out)
{
    const int b = blockIdx.z;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= W) return;
    const CropMap m = make_map(dims, com[3 * b], com[3 * b + 1], b, W, Hh, crop_w, crop_h);
    const float* __restrict__ f = flux + (int64_t)b * Hh * W;
    const CropAxis col = crop_column(m, j);
    const int i_end = min((int)(blockIdx.y + 1) * kCropRows, Hh);
    for (int i = blockIdx.y * kCropRows; i < i_end; ++i) {
        CropTaps v;
        out[(int64_t)b * Hh * W + i * W + j] = crop_sample(f, m, col, i, v);
    }
}

// gcom[b] = (dL/dxc, dL/dyc)
__global__ __launch_bounds__(kReduceBlock) void flux_crop_bwd_com_kernel(const float* __restrict__ flux,
                                                                       const float* __restrict__ dims,
                                                                       const float* __restrict__ com,
                                                                       const float* __restrict__ grad_out, int Hh, int W,
                                                                       float crop_w, float crop_h,
                                                                       float* __restrict__ gcom)
{
    __shared__ double s_red[16];
    const int b = blockIdx.x;
    const CropMap m = make_map(dims, com[3 * b], com[3 * b + 1], b, W, Hh, crop_w, crop_h);
    const float* __restrict__ f = flux + (int64_t)b * Hh * W;
    const float* __restrict__ g = grad_out + (int64_t)b * Hh * W;
    double gx = 0.0, gy = 0.0;
    // Four pixels per trip, their twenty loads issued before the first is used: one workgroup per bitmap leaves the
    // memory system nearly idle on a small field, so the loop lives on loads in flight (47 -> 20 us for 125 bitmaps).
    // The per-thread summation order is that of the one-pixel loop: results do not change.
    constexpr int U = 4;
    const int npx = Hh * W;
    for (int k0 = threadIdx.x; k0 < npx; k0 += U * blockDim.x) {
        CropTaps v[U];
        float go[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int k = k0 + q * blockDim.x;
            const bool live = k < npx;
            const int i = live ? k / W : 0, j = live ? k - i * W : 0;
            CropAxis col = crop_column(m, j);
            col.a = live && col.a; col.b = live && col.b;           // (a trip's pixels past the end load nothing)
            crop_sample(f, m, col, i, v[q]);
            go[q] = live ? g[k] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            if (k0 + q * (int)blockDim.x >= npx) break;
            float sx, sy;
            crop_sample_gradient(v[q], sx, sy);
            gx += (double)(go[q] * sx);
            gy += (double)(go[q] * sy);
        }
    }
    gx = block_sum(gx, s_red);
    gy = block_sum(gy, s_red);
    if (threadIdx.x == 0) finish_centre_gradient(gx, gy, W, Hh, gcom + 2 * b);
}

// Weight with which output pixel `o` (sampling coordinate c = map(o)) read input pixel `p`.
__device__ __forceinline__ float tap(float c, int p)
{
    const float c0 = floorf(c);
    const int p0 = (int)c0;
    const float t = c - c0;
    return p == p0 ? 1.0f - t : (p == p0 + 1 ? t : 0.0f);
}

// sum_i wy(i) sum_q wx[q] g[i, j0 + q] with the K column weights held in registers
template <int K>
__device__ __forceinline__ float gather_rows(const CropMap& m, const float* __restrict__ g, int W, int x, int y, int j0,
                                             int j1, int i0, int i1)
{
    float wx[K];
#pragma unroll
    for (int q = 0; q < K; ++q) wx[q] = j0 + q <= j1 ? tap(m.ix(j0 + q), x) : 0.0f;
    float acc = 0.0f;
    for (int i = i0; i <= i1; ++i) {
        const float wy = tap(m.iy(i), y);
        if (wy == 0.0f) continue;
        const float* __restrict__ grow = g + i * W + j0;
        float row = 0.0f;
#pragma unroll
        for (int q = 0; q < K; ++q)
            if (wx[q] != 0.0f) row += grow[q] * wx[q];
        acc += row * wy;
    }
    return acc;
}

// Candidate output indices whose sampling coordinate can lie within one pixel of input index `p`:
// ix(j) = sx (j - (W-1)/2) + (xc + 1)(W-1)/2 up to rounding (<< 1e-3 pixel for bitmaps up to 32768 wide), so the candidates
// are the j with |ix(j) - x| < 1 + 4e-3; tap() decides exactly
__device__ __forceinline__ void tap_range(float scale, float centre, int n, int p, int& lo_i, int& hi_i)
{
    lo_i = 0; hi_i = n - 1;
    if (scale > 1e-6f && scale < 1e6f) {
        const float b = (centre + 1.0f) * 0.5f * (float)(n - 1) - scale * 0.5f * (float)(n - 1);
        const float lo = ((float)p - 1.004f - b) / scale, hi = ((float)p + 1.004f - b) / scale;
        if (lo > -2.0e9f && lo < 2.0e9f && hi > -2.0e9f && hi < 2.0e9f) { lo_i = max(0, (int)ceilf(lo)); hi_i = min(n - 1, (int)floorf(hi)); }
    }
}

// Gradient of one INPUT pixel (x, y): direct part = sum over the output pixels that sampled it (the map is separable
// and monotone, so they form a small index rectangle), plus the part through the centre of mass.  General form, any
// crop scale; the tiled kernel below uses it for bitmaps whose scale needs more than four taps per axis.
__device__ __forceinline__ float crop_bwd_pixel(const CropMap& m, const float* __restrict__ g, float S,
                                                const float* __restrict__ gcom, int b, int Hh, int W, int x, int y)
{
    int j0, j1, i0, i1;
    tap_range(m.sx, m.xc, W, x, j0, j1);
    tap_range(m.sy, m.yc, Hh, y, i0, i1);
    float acc = 0.0f;
    if (j1 - j0 < 4) acc = gather_rows<4>(m, g, W, x, y, j0, j1, i0, i1);
    else if (j1 - j0 < 8) acc = gather_rows<8>(m, g, W, x, y, j0, j1, i0, i1);
    else {
        for (int i = i0; i <= i1; ++i) {
            const float wy = tap(m.iy(i), y);
            if (wy == 0.0f) continue;
            float row = 0.0f;
            for (int j = j0; j <= j1; ++j) {
                const float wx = tap(m.ix(j), x);
                if (wx != 0.0f) row += g[i * W + j] * wx;
            }
            acc += row * wy;
        }
    }
    return acc + gcom[2 * b] * (lin11(x, W) - m.xc) / S + gcom[2 * b + 1] * (lin11(y, Hh) - m.yc) / S;
}

// The same gradient organised by tiles of 64 x 32 input pixels: the map is separable, so the
// first output index and the (at most four) weights of a column are shared by the 16 pixels of that column and those
// of a row by its 64 pixels - they are computed once per tile into LDS - and the sum factorises into a horizontal
// pass (4 global loads per output row and column, kept in LDS) and a vertical pass (4 LDS reads per pixel).  A bitmap
// whose crop scale needs more than four taps per axis (scale below 0.5: tap_range's interval is 2.008 / scale output indices
// long, a fifth candidate fits from 4 on) takes the per-pixel form.
constexpr int kTileX = 64, kTileY = 32, kTaps = 4, kTileRows = 64, kRowUnroll = 4;
// LOSS = true: the fused crop + PixelLoss adjoint.  grad_out is then the RESIDUAL crop - truth that the forward pass kept, gcom
// the gradient of the two centre coordinates per unit of 2 gl / sum(truth), and the whole pixel is scaled by that factor at
// the end (everything here is linear in it): dL/dflux in ONE pass over the residual - no second sampling of the crop, no
// dL/dcrop written and read back (round 3: two kernels, 188 + 297 us at 1000 bitmaps).  com is then the forward's record
// [B,4] = (x centre, y centre, sum + 1e-8, sum of the measured flux).
template <bool LOSS>
__global__ __launch_bounds__(256) void flux_crop_bwd_tiled_kernel(const float* __restrict__ dims, const float* __restrict__ com,
                                                                  const float* __restrict__ gcom,
                                                                  const float* __restrict__ grad_out, int Hh, int W,
                                                                  float crop_w, float crop_h, float* __restrict__ grad_flux,
                                                                  const float* __restrict__ grad_loss, int grad_loss_stride)
{
    constexpr int CS = LOSS ? 4 : 3;                 // stride of the centre record
    __shared__ int s_j0[kTileX], s_i0[kTileY];
    __shared__ float s_wx[kTileX][kTaps], s_wy[kTileY][kTaps];
    __shared__ float s_t[kTileRows][kTileX];        // horizontal pass: T[i][x] = sum_q wx[x][q] g[i][j0(x) + q]
    __shared__ int s_wide, s_ilo, s_ihi;
    __shared__ float s_gy[kTileY];                   // the row's share of the centre-of-mass term (one division per row, not per pixel)
    const int b = blockIdx.z;
    const int x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY;
    const CropMap m = make_map(dims, com[CS * b], com[CS * b + 1], b, W, Hh, crop_w, crop_h);
    const float S = com[CS * b + 2];
    const float scale = LOSS ? (grad_loss[(int64_t)b * grad_loss_stride] * 2.0f) / com[CS * b + 3] : 1.0f;     // (stride 0: the gradient of a summed loss)
    if (threadIdx.x == 0) { s_wide = 0; s_ilo = 0x7fffffff; s_ihi = -1; }
    __syncthreads();
    if (threadIdx.x < kTileX + kTileY) {
        const bool col = threadIdx.x < kTileX;
        const int t = col ? threadIdx.x : threadIdx.x - kTileX;
        const int p = col ? x0 + t : y0 + t;
        const int n = col ? W : Hh;
        int lo_i = 0, hi_i = -1;
        if (p < n) tap_range(col ? m.sx : m.sy, col ? m.xc : m.yc, n, p, lo_i, hi_i);
        if (hi_i - lo_i >= kTaps) s_wide = 1;
        (col ? s_j0 : s_i0)[t] = lo_i;
        for (int q = 0; q < kTaps; ++q) {
            const int o = lo_i + q;
            (col ? s_wx[t] : s_wy[t])[q] = o <= hi_i ? tap(col ? m.ix(o) : m.iy(o), p) : 0.0f;
        }
        if (!col && hi_i >= lo_i) { atomicMin(&s_ilo, lo_i); atomicMax(&s_ihi, hi_i); }
        if (!col) s_gy[t] = gcom[2 * b + 1] * (lin11(p, Hh) - m.yc) / S;
    }
    __syncthreads();
    const int ilo = s_ilo, ihi = s_ihi;
    const float* __restrict__ g = grad_out + (int64_t)b * Hh * W;
    if (s_wide || ihi - ilo >= kTileRows) {    // strong magnification: per-pixel form for this tile
        for (int k = threadIdx.x; k < kTileX * kTileY; k += 256) {
            const int x = x0 + (k & (kTileX - 1)), y = y0 + k / kTileX;
            if (x < W && y < Hh) grad_flux[((int64_t)b * Hh + y) * W + x] = scale * crop_bwd_pixel(m, g, S, gcom, b, Hh, W, x, y);
        }
        return;
    }
    const int tx = threadIdx.x & (kTileX - 1);
    const int x = x0 + tx;
    const bool in_x = x < W;
    const int j0 = s_j0[tx];
    const float wx0 = s_wx[tx][0], wx1 = s_wx[tx][1], wx2 = s_wx[tx][2], wx3 = s_wx[tx][3];
    const int c0 = min(j0, W - 1), c1 = min(j0 + 1, W - 1), c2 = min(j0 + 2, W - 1), c3 = min(j0 + 3, W - 1);   // weight 0 there
    // horizontal pass over the output rows this tile's input rows sampled from
    // (all four taps are loaded and weighted unconditionally - absent taps have weight 0 and a clamped, valid index - so
    //  that the loads of several rows are in flight together: with a branch per tap every load was waited for in turn
    //  and a workgroup took 26 us for 6 000 loads)
    const int xr = in_x ? 1 : 0;
    auto horizontal_pass = [&](auto&& row_sum) {            // row_sum(row of g) = sum_q wx[q] row[j0 + q]
        for (int r = threadIdx.x / kTileX; r <= ihi - ilo; r += kRowUnroll * (256 / kTileX)) {
            float v[kRowUnroll];
#pragma unroll
            for (int q = 0; q < kRowUnroll; ++q) {
                const int rr = min(r + q * (256 / kTileX), ihi - ilo);
                v[q] = row_sum(g + (int64_t)(ilo + rr) * W);
            }
#pragma unroll
            for (int q = 0; q < kRowUnroll; ++q) {
                const int rr = r + q * (256 / kTileX);
                if (rr <= ihi - ilo) s_t[rr][tx] = in_x ? v[q] : 0.0f;
            }
        }
    };
    if (W >= 4) {
        // the four taps of a row are four consecutive floats: ONE 16-byte load at 4-byte alignment (from column min(j0, W - 4);
        // the weights move with it - absent taps carry weight 0 - so the non-zero products are added in the same order: same bits)
        struct __attribute__((packed, aligned(4))) Taps { float t0, t1, t2, t3; };
        const int cb = in_x ? min(j0, W - 4) : 0, sh = in_x ? j0 - cb : 0;
        const float w0 = sh == 0 ? wx0 : 0.0f, w1 = sh == 0 ? wx1 : (sh == 1 ? wx0 : 0.0f);
        const float w2 = sh == 0 ? wx2 : (sh == 1 ? wx1 : (sh == 2 ? wx0 : 0.0f));
        const float w3 = sh == 0 ? wx3 : (sh == 1 ? wx2 : (sh == 2 ? wx1 : wx0));
        horizontal_pass([&](const float* __restrict__ row) {
            const Taps t = *reinterpret_cast<const Taps*>(row + cb);
            return ((t.t0 * w0 + t.t1 * w1) + t.t2 * w2) + t.t3 * w3;
        });
    } else {
        horizontal_pass([&](const float* __restrict__ row) {
            return ((row[c0 * xr] * wx0 + row[c1 * xr] * wx1) + row[c2 * xr] * wx2) + row[c3 * xr] * wx3;
        });
    }
    __syncthreads();
    if (!in_x) return;
    const float gx = gcom[2 * b] * (lin11(x, W) - m.xc) / S;
    for (int ty = threadIdx.x / kTileX; ty < kTileY; ty += 256 / kTileX) {
        const int y = y0 + ty;
        if (y >= Hh) break;
        const int r0 = s_i0[ty] - ilo;
        float acc = 0.0f;
#pragma unroll
        for (int a = 0; a < kTaps; ++a) {
            const float wy = s_wy[ty][a];
            if (wy != 0.0f) acc += s_t[r0 + a][tx] * wy;      // uniform across the 64 lanes of a row
        }
        acc += gx + s_gy[ty];
        grad_flux[((int64_t)b * Hh + y) * W + x] = LOSS ? scale * acc : acc;
    }
}

// ---------------------------------------------------------------------------------------------------
// Losses: one workgroup per sample.  mode 0 = PixelLoss, 1 = KLDivergenceLoss.
// ---------------------------------------------------------------------------------------------------
// Element loop over one sample with four elements per load when the sample is 16-byte aligned: fewer, wider loads
// in flight per thread (a sample is streamed by ONE workgroup, so the loop is latency-bound when B is small).
template <typename F>
__device__ __forceinline__ void for_each_pair(const float* __restrict__ p, const float* __restrict__ g, int64_t npix, F&& f)
{
    const bool vec = (npix & 3) == 0 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g)) & 15) == 0;
    if (vec) {
        const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
        for (int64_t k = threadIdx.x; k < (npix >> 2); k += blockDim.x) {
            const float4 a = p4[k], c = g4[k];
            f(4 * k, a.x, c.x); f(4 * k + 1, a.y, c.y); f(4 * k + 2, a.z, c.z); f(4 * k + 3, a.w, c.w);
        }
    } else {
        for (int64_t k = threadIdx.x; k < npix; k += blockDim.x) f(k, p[k], g[k]);
    }
}

// KLDivergenceLoss (loss.py:385-410) of a prediction p against a truth g, both L1-normalised with a clamped norm:
// sum_k exp(t_k) (t_k - q_k) with t = log(g / dg + eps), q = log(p / dp + eps).  `term` adds a pixel's share of the loss and of
// dot = sum_k a_k p_k, a_k = -exp(t_k) / (p_k / dp + eps); `gradient` is gl dKL/dp_k, the second part through the norm of p.
struct KlNorms {
    static constexpr float eps = 1e-12f;
    float npf, ngf, dp, dg;
    __device__ __forceinline__ KlNorms(float np_, float ng_) : npf(np_), ngf(ng_), dp(fmaxf(np_, eps)), dg(fmaxf(ng_, eps)) {}
    __device__ __forceinline__ void term(float pk, float gk, double& acc, double& dot) const
    {
        const float t = logf(gk / dg + eps), q = logf(pk / dp + eps);
        const float et = expf(t);
        acc += (double)(et * (t - q));
        dot += (double)((-et / (pk / dp + eps)) * pk);
    }
    __device__ __forceinline__ float gradient(float pk, float gk, float dotf, float gl) const
    {
        const float t = logf(gk / dg + eps);
        const float a = -expf(t) / (pk / dp + eps);
        const float sgn = pk > 0.0f ? 1.0f : (pk < 0.0f ? -1.0f : 0.0f);
        const float through_norm = npf > eps ? sgn * dotf / (dp * dp) : 0.0f;
        return gl * (a / dp - through_norm);
    }
};

__global__ __launch_bounds__(kReduceBlock) void flux_loss_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                               int64_t npix, int mode, float* __restrict__ loss,
                                                               const float* __restrict__ grad_loss,
                                                               float* __restrict__ grad_pred)
{
    __shared__ double s_red[16];
    const int b = blockIdx.x;
    const float* __restrict__ p = pred + (int64_t)b * npix;
    const float* __restrict__ g = truth + (int64_t)b * npix;
    float* __restrict__ gp = grad_pred ? grad_pred + (int64_t)b * npix : nullptr;
    if (mode == 0) {                                           // loss.py:312-318
        double se = 0.0, sg = 0.0;
        for_each_pair(p, g, npix, [&](int64_t, float pk, float gk) { const float d = pk - gk; se += (double)(d * d); sg += (double)gk; });
        se = block_sum(se, s_red);
        const float sgf = (float)block_sum(sg, s_red);
        if (threadIdx.x == 0 && loss) loss[b] = (float)se / sgf;
        if (gp) {
            const float gl = grad_loss[b];
            for_each_pair(p, g, npix, [&](int64_t k, float pk, float gk) { gp[k] = gl * (2.0f * (pk - gk)) / sgf; });
        }
        return;
    }
    double np_ = 0.0, ng = 0.0;
    for_each_pair(p, g, npix, [&](int64_t, float pk, float gk) { np_ += (double)fabsf(pk); ng += (double)fabsf(gk); });
    const float npf = (float)block_sum(np_, s_red), ngf = (float)block_sum(ng, s_red);
    const KlNorms kl(npf, ngf);
    double acc = 0.0, dot = 0.0;
    for_each_pair(p, g, npix, [&](int64_t, float pk, float gk) { kl.term(pk, gk, acc, dot); });
    acc = block_sum(acc, s_red);
    const float dotf = (float)block_sum(dot, s_red);
    if (threadIdx.x == 0 && loss) loss[b] = (float)acc;
    if (gp) {
        const float gl = grad_loss[b];
        for_each_pair(p, g, npix, [&](int64_t k, float pk, float gk) { gp[k] = kl.gradient(pk, gk, dotf, gl); });
    }
}

// ---------------------------------------------------------------------------------------------------
// The gain-free kinds of art_flux_loss (include/artist_hip.h): 2 Jensen-Shannon, 3 shape pixel loss, 4 total variation on the
// L1-normalised bitmaps p^ = p / dp, g^ = g / dg (norms and clamps as KlNorms forms them), 5 one minus the cosine similarity.
// Kernels of their own, one per kind: flux_loss_kernel and its registers stay what they were.  Same shape as kind 1 - one
// workgroup per bitmap, fp64 per-thread sums in for_each_pair's order, the block tree, no atomics: a bitmap's bits depend on
// neither the batch nor the run.  The sums are over pixels that are formed again in the gradient pass (nothing is kept).
// ---------------------------------------------------------------------------------------------------
// One pixel of kinds 2 to 4: its share of the loss sum (before the kind's factor, see unit_l1_loss_factor) and a = dL/dp^_k.
template <int KIND>
__device__ __forceinline__ double unit_l1_pixel(float ph, float gh, float pixels, float& a)
{
    constexpr float eps = KlNorms::eps;
    if constexpr (KIND == 2) {
        // 1/2 sum u (log u - log w) + 1/2 sum v (log v - log w), u = g^ + eps, v = p^ + eps, w = (p^ + g^) / 2 + eps.  w moves
        // by half of p^, and u + v = 2 w: what is left of the derivative is (log v - log w) / 2.
        const float u = gh + eps, v = ph + eps;
        const float lw = logf(0.5f * (ph + gh) + eps);
        const float du = logf(u) - lw, dv = logf(v) - lw;
        a = 0.5f * dv;
        return (double)(u * du) + (double)(v * dv);
    } else {
        const float d = ph - gh;
        if constexpr (KIND == 3) {
            a = (2.0f * pixels) * d;
            return (double)(d * d);
        } else {
            a = d > 0.0f ? 0.5f : (d < 0.0f ? -0.5f : 0.0f);        // (|x| has derivative 0 at 0, as torch's abs)
            return (double)fabsf(d);
        }
    }
}
template <int KIND>
__device__ __forceinline__ double unit_l1_loss_factor(int64_t npix) { return KIND == 3 ? (double)npix : 0.5; }

// gl dL/dp_k of a loss of p^ from a_k = dL/dp^_k and dot = sum_j a_j p_j: the pixel's own part and the part through the norm of p
// (sign(p_k) dot / dp^2; none when the norm is clamped).  Divided by dp twice: dp^2 would leave fp32 for norms beyond 1e19.
__device__ __forceinline__ float unit_l1_gradient(const KlNorms& n, float a, float pk, float dotf, float gl)
{
    const float sgn = pk > 0.0f ? 1.0f : (pk < 0.0f ? -1.0f : 0.0f);
    const float through_norm = n.npf > KlNorms::eps ? sgn * ((dotf / n.dp) / n.dp) : 0.0f;
    return gl * (a / n.dp - through_norm);
}

template <int KIND>
__global__ __launch_bounds__(kReduceBlock) void flux_gain_free_loss_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                                         int64_t npix, float* __restrict__ loss,
                                                                         const float* __restrict__ grad_loss,
                                                                         float* __restrict__ grad_pred)
{
    __shared__ double s_red[16 * 3];
    const int b = blockIdx.x;
    const float* __restrict__ p = pred + (int64_t)b * npix;
    const float* __restrict__ g = truth + (int64_t)b * npix;
    float* __restrict__ gp = grad_pred ? grad_pred + (int64_t)b * npix : nullptr;
    if constexpr (KIND == 5) {
        // torch.nn.functional.cosine_similarity (eps = 1e-8): sum (p / max(|p|_2, eps)) (g / max(|g|_2, eps)) - EACH norm is clamped,
        // and the clamp is applied outside autograd: the gradient goes through |p|_2 as if it were not clamped (0 at p = 0).
        // The three sums of one pass give the same number: dot / (n1c n2c).
        constexpr float eps = 1e-8f;
        double pp = 0.0, gg = 0.0, pg = 0.0;
        for_each_pair(p, g, npix, [&](int64_t, float pk, float gk) { pp += (double)(pk * pk); gg += (double)(gk * gk); pg += (double)(pk * gk); });
        double s[3] = {pp, gg, pg};
        block_sum_n<3>(s, s_red);
        const float n1 = (float)sqrt(s[0]), n2 = (float)sqrt(s[1]);
        const float n1c = fmaxf(n1, eps), n2c = fmaxf(n2, eps);
        const float c = (float)s[2] / (n1c * n2c);
        if (threadIdx.x == 0 && loss) loss[b] = 1.0f - c;
        if (gp) {
            // d(1 - c)/dp_k = -(g_k / n2c - c p_k / |p|_2) / n1c
            const float gl = grad_loss[b];
            for_each_pair(p, g, npix, [&](int64_t k, float pk, float gk) {
                const float along = n1 > 0.0f ? pk / n1 : 0.0f;
                gp[k] = -gl * ((gk / n2c - c * along) / n1c);
            });
        }
    } else {
        double np_ = 0.0, ng = 0.0;
        for_each_pair(p, g, npix, [&](int64_t, float pk, float gk) { np_ += (double)fabsf(pk); ng += (double)fabsf(gk); });
        double norms[2] = {np_, ng};
        block_sum_n<2>(norms, s_red);
        const KlNorms n((float)norms[0], (float)norms[1]);
        const float pixels = (float)npix;
        double acc = 0.0, dot = 0.0;
        for_each_pair(p, g, npix, [&](int64_t, float pk, float gk) {
            float a;
            acc += unit_l1_pixel<KIND>(pk / n.dp, gk / n.dg, pixels, a);
            dot += (double)(a * pk);
        });
        double s[2] = {acc, dot};
        block_sum_n<2>(s, s_red);
        const float dotf = (float)s[1];
        if (threadIdx.x == 0 && loss) loss[b] = (float)(s[0] * unit_l1_loss_factor<KIND>(npix));
        if (gp) {
            const float gl = grad_loss[b];
            for_each_pair(p, g, npix, [&](int64_t k, float pk, float gk) {
                float a;
                unit_l1_pixel<KIND>(pk / n.dp, gk / n.dg, pixels, a);
                gp[k] = unit_l1_gradient(n, a, pk, dotf, gl);
            });
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// The fused crop + PixelLoss pair.  A bitmap's rows are ALWAYS summed in kLossParts = 4 parts, whatever the batch size: the
// parts' fp64 sums (per-thread order, block tree) are added in part order, so the loss, the centre and the gradient are the
// same bits whether a bitmap has one workgroup (large batches: all four parts in one workgroup, one launch) or two / four
// (small batches - one of eight ranks' 125 bitmaps on 256 CUs; as many workgroups as still have a CU each, the parts
// carried from kernel to kernel through a small scratch).  Round 3's one-workgroup kernels summed all rows in one go and
// differed from the part kernels in the last bits: the same data gave another loss at another batch size (advisor).
//   flux_com_parts_kernel           grid (P, B): the centre-of-mass sums of each part -> parts[b][v][0..2]       (P > 1 only)
//   flux_crop_pixel_loss_fwd_kernel grid (P, B): [P == 1: the same sums first, in the workgroup] the four parts in part order
//                                   -> the centre; crops and compares its parts' rows; per part (sum d^2, sum truth) and -
//                                   when a backward pass will follow - the RESIDUAL d = crop - truth [B,Hh,W] and the two
//                                   sums that make the gradient of the centre; [P == 1: loss and records written here]
//   flux_crop_pixel_loss_final_kernel  one thread per bitmap adds the parts                                      (P > 1 only)
//   backward                        flux_crop_bwd_tiled_kernel<true>: ONE pass over the residual (see there)
// (A "last workgroup adds the parts" ticket was built first: its device-scope fences write back and invalidate the L2 of
//  every XCD - 0.24 instead of 0.04 ms at 125 bitmaps.  Kernel boundaries carry the parts instead.)
// ---------------------------------------------------------------------------------------------------
constexpr int kMaxPartBitmaps = 512;
struct PartScratch { double com[kMaxPartBitmaps][kLossParts][3]; double acc[kMaxPartBitmaps][kLossParts][4]; };

__global__ __launch_bounds__(kReduceBlock) void flux_com_parts_kernel(const float* __restrict__ flux, int Hh, int W, int parts_per_wg,
                                                                    PartScratch* __restrict__ ws)
{
    __shared__ double s_red[16 * 4];
    const int b = blockIdx.y;
    const float* __restrict__ f = flux + (int64_t)b * Hh * W;
    for (int v = blockIdx.x * parts_per_wg; v < (int)(blockIdx.x + 1) * parts_per_wg; ++v) {
        double a[3];
        com_part_sums(f, Hh, W, v, s_red, a);
        if (threadIdx.x == 0) { ws->com[b][v][0] = a[0]; ws->com[b][v][1] = a[1]; ws->com[b][v][2] = a[2]; }
    }
}

// the centre of a bitmap from its four parts (part order); every workgroup of the bitmap computes the same three numbers
__device__ __forceinline__ void com_from_parts(const double (*parts)[3], float& xc, float& yc, float& S)
{
    double s = 0.0, xs = 0.0, ys = 0.0;
    for (int v = 0; v < kLossParts; ++v) { s += parts[v][0]; xs += parts[v][1]; ys += parts[v][2]; }
    centre_from_sums(s, xs, ys, xc, yc, S);
}

// loss, the record the backward pass reads and - with a residual - the centre's gradient per unit of 2 gl / sum(truth)
__device__ __forceinline__ void loss_from_parts(const double (*acc)[4], float xc, float yc, float S, int b, int Hh, int W,
                                                float* __restrict__ loss, float* __restrict__ com4, float* __restrict__ gunit)
{
    double se = 0.0, sg = 0.0, gx = 0.0, gy = 0.0;
    for (int v = 0; v < kLossParts; ++v) { se += acc[v][0]; sg += acc[v][1]; gx += acc[v][2]; gy += acc[v][3]; }
    const float sgf = (float)sg;
    loss[b] = (float)se / sgf;                              // loss.py:312-318
    com4[4 * b] = xc; com4[4 * b + 1] = yc; com4[4 * b + 2] = S; com4[4 * b + 3] = sgf;
    if (gunit) finish_centre_gradient(gx, gy, W, Hh, gunit + 2 * b);
}

template <bool WHOLE>       // WHOLE: one workgroup per bitmap does all four parts, the centre and the final sums itself
__global__ __launch_bounds__(kReduceBlock) void flux_crop_pixel_loss_fwd_kernel(const float* __restrict__ flux,
                                                                               const float* __restrict__ dims,
                                                                               const float* __restrict__ truth, int Hh, int W,
                                                                               float crop_w, float crop_h, int parts_per_wg,
                                                                               PartScratch* ws, float* __restrict__ residual,
                                                                               float* __restrict__ loss, float* __restrict__ com4,
                                                                               float* __restrict__ gunit, const double* __restrict__ moments,
                                                                               int stage_rows)
{
    extern __shared__ __attribute__((aligned(16))) float s_stage[];      // stage_rows x W floats (see the column loop)
    __shared__ double s_red[16 * 4];
    __shared__ double s_com[kLossParts][3], s_acc[kLossParts][4];
    const int b = blockIdx.y;
    const float* __restrict__ f = flux + (int64_t)b * Hh * W;
    const float* __restrict__ g = truth + (int64_t)b * Hh * W;
    float* __restrict__ res = residual ? residual + (int64_t)b * Hh * W : nullptr;
    float xc, yc, S;
    if (moments != nullptr) {          // the sums came with the bitmaps (the trace's conversion pass formed them: flux_moments.hpp)
        com_from_parts(reinterpret_cast<const double(*)[3]>(moments + (int64_t)b * kLossParts * 3), xc, yc, S);
    } else if constexpr (WHOLE) {
        for (int v = 0; v < kLossParts; ++v) {
            double a[3];
            com_part_sums(f, Hh, W, v, s_red, a);
            if (threadIdx.x == 0) { s_com[v][0] = a[0]; s_com[v][1] = a[1]; s_com[v][2] = a[2]; }
        }
        __syncthreads();
        com_from_parts(s_com, xc, yc, S);
    } else {
        com_from_parts(ws->com[b], xc, yc, S);
    }
    const CropMap m = make_map(dims, xc, yc, b, W, Hh, crop_w, crop_h);
    for (int v = blockIdx.x * parts_per_wg; v < (int)(blockIdx.x + 1) * parts_per_wg; ++v) {
        int r0, r1;
        part_rows(Hh, v, r0, r1);
        double a[4] = {0.0, 0.0, 0.0, 0.0};             // sum d^2, sum truth, and the two sums of the centre's gradient
        if ((int)blockDim.x % W == 0) {                 // a thread owns one column
            const int j = threadIdx.x % W, di = blockDim.x / W;
            const CropAxis col = crop_column(m, j);
            // The bitmap rows this part's output rows sample, staged in LDS with 16-byte loads when they fit (stage_rows of them:
            // the launch's dynamic LDS): the four taps of a pixel are then LDS reads - a fifth of the vector-memory instructions
            // (four predicated 4-byte taps per pixel were four tag look-ups of the same two cache lines per wave): 0.298 -> 0.257 ms
            // per 1000 bitmaps.  Same values, same arithmetic: same bits.
            int ylo = 0, nrows = 0;
            if (stage_rows > 0 && (W & 3) == 0) {
                const float ya_ = m.iy(r0), yb_ = m.iy(r1 - 1);
                if (ya_ > -1.0e9f && ya_ < 1.0e9f && yb_ > -1.0e9f && yb_ < 1.0e9f) {
                    ylo = max(0, (int)floorf(fminf(ya_, yb_)));
                    const int yhi = min(Hh - 1, (int)floorf(fmaxf(ya_, yb_)) + 1);
                    nrows = yhi - ylo + 1;
                    if (nrows > stage_rows) nrows = 0;
                }
            }
            // four rows per step, every tap and the measured flux loaded BEFORE the first residual is stored: the loop is a chain
            // of L2 round trips otherwise (a store between two rows' loads keeps the compiler from having them in flight together)
            constexpr int kRows = 4;
            auto rows = [&](auto&& pixel) {
            for (int i0 = r0 + threadIdx.x / W; i0 < r1; i0 += kRows * di) {
                float c[kRows], t[kRows], gxs[kRows], gys[kRows];
#pragma unroll
                for (int u = 0; u < kRows; ++u) {
                    const int i = min(i0 + u * di, r1 - 1);                 // (a clamped row is loaded and not used)
                    CropTaps v;
                    c[u] = crop_sample_from(pixel, m, col, i, v);
                    t[u] = g[i * W + j];
                    crop_sample_gradient(v, gxs[u], gys[u]);
                }
#pragma unroll
                for (int u = 0; u < kRows; ++u) {
                    const int i = i0 + u * di;
                    if (i >= r1) break;
                    const float d = c[u] - t[u];
                    a[0] += (double)(d * d); a[1] += (double)t[u];
                    if (res) {
                        res[i * W + j] = d;
                        a[2] += (double)(d * gxs[u]);
                        a[3] += (double)(d * gys[u]);
                    }
                }
            }
            };
            if (nrows > 0) {                            // (workgroup-uniform)
                __syncthreads();                        // the previous part's readers are done with the staged rows
                const float4* __restrict__ src = reinterpret_cast<const float4*>(f + (int64_t)ylo * W);
                float4* dst = reinterpret_cast<float4*>(s_stage);
                for (int k = threadIdx.x; k < nrows * (W >> 2); k += blockDim.x) dst[k] = src[k];
                __syncthreads();
                const float* staged = s_stage - ylo * W;      // (row y of the bitmap at staged + y W)
                rows([&](int k) { return staged[k]; });
            } else {
                rows([&](int k) { return f[k]; });
            }
        } else {
            for (int k = r0 * W + threadIdx.x; k < r1 * W; k += blockDim.x) {
                const int i = k / W, j = k - i * W;
                CropTaps v;
                const float c = crop_sample(f, m, crop_column(m, j), i, v);
                const float t = g[k];
                const float d = c - t;
                a[0] += (double)(d * d); a[1] += (double)t;
                if (res) {
                    float gxs, gys;
                    crop_sample_gradient(v, gxs, gys);
                    res[k] = d;
                    a[2] += (double)(d * gxs);
                    a[3] += (double)(d * gys);
                }
            }
        }
        block_sum_n<4>(a, s_red);
        if (threadIdx.x == 0) {
            double* out = WHOLE ? s_acc[v] : ws->acc[b][v];
            out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
        }
    }
    if constexpr (WHOLE) {
        if (threadIdx.x == 0) loss_from_parts(s_acc, xc, yc, S, b, Hh, W, loss, com4, gunit);     // (its own writes)
    }
}

// the parts of the bitmaps that were shared among workgroups -> loss and records: one thread per bitmap
__global__ __launch_bounds__(256) void flux_crop_pixel_loss_final_kernel(const PartScratch* __restrict__ ws, int B, int Hh, int W,
                                                                         float* __restrict__ loss, float* __restrict__ com4,
                                                                         float* __restrict__ gunit, const double* __restrict__ moments)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float xc, yc, S;
    com_from_parts(moments ? reinterpret_cast<const double(*)[3]>(moments + (int64_t)b * kLossParts * 3) : ws->com[b], xc, yc, S);
    loss_from_parts(ws->acc[b], xc, yc, S, b, Hh, W, loss, com4, gunit);
}

// get_center_of_mass backward, one elementwise pass: d e_com / d f_ij = (j - e_com) / (S + 1e-8)
__global__ __launch_bounds__(kFluxBlock) void flux_com_px_bwd_kernel(const float* __restrict__ com, const float* __restrict__ grad_com,
                                                                     int Hh, int W, float* __restrict__ grad_flux)
{
    const int b = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Hh * W) return;
    const int i = k / W, j = k - i * W;
    const float S = com[3 * b + 2];
    grad_flux[(int64_t)b * Hh * W + k] = (grad_com[2 * b] * ((float)j - com[3 * b]) + grad_com[2 * b + 1] * ((float)i - com[3 * b + 1])) / S;
}

// ---------------------------------------------------------------------------------------------------
// Fused crop around the centre of mass + KLDivergenceLoss (artist/flux/bitmap.py:121-246 followed by
// artist/optim/loss.py:321-410 with the reduction over the two bitmap dimensions), one workgroup per bitmap: the cropped
// bitmap never reaches HBM.  The KL terms need the crop's L1 norm first, so the crop is sampled twice (the taps hit L2: the
// workgroup has just streamed the bitmap).  rec8[b] = (x centre, y centre, sum + 1e-8, |crop|_1, |truth|_1, dot, 0, 0) for
// the backward pass (dot: see KlNorms).
// ---------------------------------------------------------------------------------------------------
// fn(k, crop_k, its taps) for every output pixel k of the crop of bitmap `f`, each thread in its own fixed order
// (a thread owns one column when the workgroup size is a multiple of the bitmap width)
template <typename F>
__device__ __forceinline__ void for_each_crop_pixel(const float* __restrict__ f, const CropMap& m, F&& fn)
{
    const int W = m.W, Hh = m.Hh;
    auto pixel = [&](int k, int i, const CropAxis& col) {
        CropTaps v;
        const float c = crop_sample(f, m, col, i, v);
        fn(k, c, v);
    };
    if ((int)blockDim.x % W == 0) {
        const int j = threadIdx.x % W, di = blockDim.x / W;
        const CropAxis col = crop_column(m, j);
#pragma unroll 4
        for (int i = threadIdx.x / W; i < Hh; i += di) pixel(i * W + j, i, col);
    } else {
        for (int k = threadIdx.x; k < Hh * W; k += blockDim.x) {
            const int i = k / W, j = k - i * W;
            pixel(k, i, crop_column(m, j));
        }
    }
}

__global__ __launch_bounds__(kReduceBlock) void flux_crop_kl_loss_fwd_kernel(const float* __restrict__ flux,
                                                                            const float* __restrict__ dims,
                                                                            const float* __restrict__ truth, int Hh, int W,
                                                                            float crop_w, float crop_h, float* __restrict__ loss,
                                                                            float* __restrict__ rec8)
{
    __shared__ double s_red[16 * 3];
    __shared__ float s_com[3];
    const int b = blockIdx.x;
    const float* __restrict__ f = flux + (int64_t)b * Hh * W;
    const float* __restrict__ g = truth + (int64_t)b * Hh * W;
    double sums[3];
    moment_sums<NormalisedWeights>(f, Hh, W, 0, Hh, s_red, sums);
    if (threadIdx.x == 0) centre_from_sums(sums[0], sums[1], sums[2], s_com[0], s_com[1], s_com[2]);     // (two fp64 divisions: one thread)
    __syncthreads();
    const float xc = s_com[0], yc = s_com[1], S = s_com[2];
    const CropMap m = make_map(dims, xc, yc, b, W, Hh, crop_w, crop_h);
    double np_ = 0.0, ng = 0.0;
    for_each_crop_pixel(f, m, [&](int k, float c, const CropTaps&) { np_ += (double)fabsf(c); ng += (double)fabsf(g[k]); });
    const float npf = (float)block_sum(np_, s_red), ngf = (float)block_sum(ng, s_red);
    const KlNorms kl(npf, ngf);
    double acc = 0.0, dot = 0.0;
    for_each_crop_pixel(f, m, [&](int k, float c, const CropTaps&) { kl.term(c, g[k], acc, dot); });
    acc = block_sum(acc, s_red);
    const float dotf = (float)block_sum(dot, s_red);
    if (threadIdx.x == 0) {
        loss[b] = (float)acc;
        float* r = rec8 + 8 * b;
        r[0] = xc; r[1] = yc; r[2] = S; r[3] = npf; r[4] = ngf; r[5] = dotf; r[6] = 0.0f; r[7] = 0.0f;
    }
}

// grad_crop[b] = gl[b] dKL/dcrop (written), gcom[b] = its gradient w.r.t. the two centre coordinates, com3 for the tiled gather
__global__ __launch_bounds__(kReduceBlock) void flux_crop_kl_loss_bwd_kernel(const float* __restrict__ flux,
                                                                            const float* __restrict__ dims,
                                                                            const float* __restrict__ truth,
                                                                            const float* __restrict__ rec8,
                                                                            const float* __restrict__ grad_loss, int Hh, int W,
                                                                            float crop_w, float crop_h,
                                                                            float* __restrict__ grad_crop, float* __restrict__ com3,
                                                                            float* __restrict__ gcom)
{
    __shared__ double s_red[16];
    const int b = blockIdx.x;
    const float* __restrict__ f = flux + (int64_t)b * Hh * W;
    const float* __restrict__ g = truth + (int64_t)b * Hh * W;
    float* __restrict__ gc = grad_crop + (int64_t)b * Hh * W;
    const float* r = rec8 + 8 * b;
    const CropMap m = make_map(dims, r[0], r[1], b, W, Hh, crop_w, crop_h);
    const KlNorms kl(r[3], r[4]);
    const float dotf = r[5], gl = grad_loss[b];
    double gx = 0.0, gy = 0.0;
    for_each_crop_pixel(f, m, [&](int k, float c, const CropTaps& v) {
        const float go = kl.gradient(c, g[k], dotf, gl);
        float sx, sy;
        crop_sample_gradient(v, sx, sy);
        gc[k] = go;
        gx += (double)(go * sx);
        gy += (double)(go * sy);
    });
    gx = block_sum(gx, s_red);
    gy = block_sum(gy, s_red);
    if (threadIdx.x == 0) {
        finish_centre_gradient(gx, gy, W, Hh, gcom + 2 * b);
        com3[3 * b] = m.xc; com3[3 * b + 1] = m.yc; com3[3 * b + 2] = r[2];
    }
}

}  // namespace art

using namespace art;

// Scratch of the part kernels: one PartScratch per (device, stream), allocated on first use and kept (every entry is written
// before it is read: no initialisation).  nullptr when the allocation fails: the callers give a bitmap one workgroup.  nullptr as
// well, with nothing allocated, for a stream that has none yet and is being captured: the caller returns ART_EUNSUPPORTED.
static PartScratch* flux_parts_scratch(hipStream_t stream)
{
    struct Entry { int dev; hipStream_t stream; PartScratch* ws; };
    static std::vector<Entry> table;
    static std::mutex lock;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> guard(lock);
    for (const Entry& e : table)
        if (e.dev == dev && e.stream == stream) return e.ws;
    if (stream_is_capturing(stream)) return nullptr;        // (the caller reports it: no one-workgroup fall-back inside a capture)
    PartScratch* ws = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&ws), sizeof(PartScratch)) != hipSuccess) return nullptr;
    table.push_back({dev, stream, ws});
    return ws;
}

// Workgroups per bitmap of the fused crop + loss pair: as many of 4 / 2 / 1 as still leave every workgroup a CU of its own
// (the passes are bound by what ONE CU's texture path delivers: two workgroups on a CU gain nothing and the extra launches
// cost ~4 us each).  Measured, forward / backward in us (tools/flux_bench.py; 1, 2, 4 workgroups per bitmap): 64 bitmaps
// 40 / 71, 35 / 57, 22 / 45; 125 bitmaps 42 / 84, 37 / 73, 37 / 74; 180 bitmaps 43 / 98, 63 / 112, 52 / 100; 250 bitmaps
// 45 / 114, 64 / 128, 66 / 130.  (ARTIST_HIP_DEBUG=1 ARTIST_HIP_LOSS_PARTS = 1 / 2 / 4 forces a value: tests - the results are the same bits.)
static int loss_workgroups_per_bitmap(int64_t B, int64_t Hh)
{
    const int forced = debug_env_int("ARTIST_HIP_LOSS_PARTS", 0);
    if (B > kMaxPartBitmaps || Hh < kLossParts) return 1;
    if (forced == 1 || forced == 2 || forced == 4) return forced;
    int cus = 256;
    {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
            cus = n;
    }
    return 4 * B <= cus ? 4 : (2 * B <= cus ? 2 : 1);
}

template <bool LOSS>        // (see the kernel for what com, gcom and grad_out are with LOSS)
static void launch_crop_bwd_tiled(hipStream_t stream, const float* dims, const float* com, const float* gcom, const float* grad_out,
                                  int64_t B, int64_t Hh, int64_t W, double crop_width, double crop_height, float* grad_flux,
                                  const float* grad_loss = nullptr, int64_t grad_loss_stride = 1)
{
    hipLaunchKernelGGL(flux_crop_bwd_tiled_kernel<LOSS>,
                       dim3((unsigned)((W + kTileX - 1) / kTileX), (unsigned)((Hh + kTileY - 1) / kTileY), (unsigned)B),
                       dim3(256), 0, stream, dims, com, gcom, grad_out, (int)Hh, (int)W, (float)crop_width, (float)crop_height,
                       grad_flux, grad_loss, (int)grad_loss_stride);
}

// flux_blur_kernels.hip: the blur mode of art_flux_crop_fwd.
namespace art {
int flux_blur_launch(const float* x, const float* covariance, int64_t B, int64_t Hh, int64_t W, float* out, hipStream_t stream);
// ... and the blur mode of art_flux_crop_bwd: the gradient with respect to the covariances.
int flux_blur_grad_launch(const float* x, const float* covariance, const float* g, int64_t B, int64_t Hh, int64_t W, float* out,
                          hipStream_t stream);
// radial_blur_kernels.hip: its radial window mode.
int flux_radial_blur_launch(const float* x, const float* metric, const float* table, int64_t K, int64_t B, int64_t Hh, int64_t W,
                            float* out, hipStream_t stream);
}

static bool crop_args_ok(const void* a, const void* b, const void* c, const void* d, int64_t B, int64_t Hh, int64_t W)
{
    return a && b && c && d && B >= 0 && Hh >= 1 && W >= 1 && Hh <= 65535 && Hh * W <= (int64_t)1 << 30 && B <= 65535;
}

// An empty batch (a rank without an active heliostat) has nothing to launch and nothing to point at: the tensors of such a call
// are empty, and an empty tensor's data pointer is null.  ART_OK before the pointers are looked at.
static bool empty_batch(int64_t B, int64_t Hh, int64_t W)
{
    return B == 0 && Hh >= 1 && W >= 1;
}

extern "C" int art_flux_crop_fwd(const float* flux, const float* target_dims, int64_t B, int64_t Hh, int64_t W,
                                 double crop_width, double crop_height, float* out, float* centers, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (crop_width == -1.0 && crop_height == -1.0)          // blur mode: centers holds the windows' covariances and is READ
        return target_dims ? ART_EINVAL : flux_blur_launch(flux, centers, B, Hh, W, out, stream);
    if (crop_width == -2.0) {       // radial window mode: crop_height = -K, target_dims holds the quantile table, centers the metrics; both READ
        const double K = -crop_height;
        if (!(K >= 1.0 && K <= 4096.0) || K != floor(K)) return ART_EINVAL;
        return flux_radial_blur_launch(flux, centers, target_dims, (int64_t)K, B, Hh, W, out, stream);
    }
    if (empty_batch(B, Hh, W)) return ART_OK;
    if (!crop_args_ok(flux, target_dims, out, centers, B, Hh, W)) return ART_EINVAL;
    hipLaunchKernelGGL(flux_com_kernel<NormalisedWeights>, dim3((unsigned)B), dim3(kReduceBlock), 0, stream, flux, (int)Hh, (int)W, centers);
    hipLaunchKernelGGL(flux_crop_fwd_kernel,
                       dim3((unsigned)((W + kFluxBlock - 1) / kFluxBlock), (unsigned)((Hh + kCropRows - 1) / kCropRows), (unsigned)B),
                       dim3(kFluxBlock), 0, stream, flux, target_dims, centers, (int)Hh, (int)W, (float)crop_width,
                       (float)crop_height, out);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_flux_crop_bwd(const float* flux, const float* target_dims, const float* centers, int64_t B,
                                 int64_t Hh, int64_t W, double crop_width, double crop_height, const float* grad_out,
                                 float* grad_flux, float* workspace, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // blur mode: centers holds the windows' covariances and is READ, workspace [B,3] takes the gradient with respect to them
    if (crop_width == -1.0 && crop_height == -1.0 && !target_dims)
        return flux_blur_grad_launch(flux, centers, grad_out, B, Hh, W, workspace, stream);
    if (empty_batch(B, Hh, W)) return ART_OK;
    if (!crop_args_ok(flux, target_dims, centers, grad_out, B, Hh, W) || !grad_flux || !workspace) return ART_EINVAL;
    hipLaunchKernelGGL(flux_crop_bwd_com_kernel, dim3((unsigned)B), dim3(kReduceBlock), 0, stream, flux, target_dims, centers,
                       grad_out, (int)Hh, (int)W, (float)crop_width, (float)crop_height, workspace);
    launch_crop_bwd_tiled<false>(stream, target_dims, centers, workspace, grad_out, B, Hh, W, crop_width, crop_height, grad_flux);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_flux_loss(const float* prediction, const float* ground_truth, int64_t B, int64_t npix, int kind,
                             float* loss, const float* grad_loss, float* grad_prediction, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool known_kind = kind >= 0 && kind <= 5;
    if (empty_batch(B, npix, 1) && known_kind) return ART_OK;
    if (!prediction || !ground_truth || B < 0 || npix < 1 || !known_kind || (!loss && !grad_prediction) ||
        (grad_prediction && !grad_loss))
        return ART_EINVAL;
    auto gain_free = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(kReduceBlock), 0, stream, prediction, ground_truth, npix, loss, grad_loss,
                           grad_prediction);
    };
    switch (kind) {
    case 2: gain_free(flux_gain_free_loss_kernel<2>); break;
    case 3: gain_free(flux_gain_free_loss_kernel<3>); break;
    case 4: gain_free(flux_gain_free_loss_kernel<4>); break;
    case 5: gain_free(flux_gain_free_loss_kernel<5>); break;
    default:
        hipLaunchKernelGGL(flux_loss_kernel, dim3((unsigned)B), dim3(kReduceBlock), 0, stream, prediction, ground_truth, npix,
                           kind, loss, grad_loss, grad_prediction);
    }
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_flux_crop_pixel_loss_fwd(const float* flux, const float* target_dims, const float* ground_truth, int64_t B,
                                            int64_t Hh, int64_t W, double crop_width, double crop_height, float* loss,
                                            float* centers4, float* residual, float* center_grad_unit, const double* moments,
                                            void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (empty_batch(B, Hh, W)) return ART_OK;
    if (!crop_args_ok(flux, target_dims, ground_truth, loss, B, Hh, W) || !centers4 || (residual != nullptr) != (center_grad_unit != nullptr))
        return ART_EINVAL;
    const int P = loss_workgroups_per_bitmap(B, Hh);
    PartScratch* ws = P > 1 ? flux_parts_scratch(stream) : nullptr;
    if (P > 1 && ws == nullptr && stream_is_capturing(stream)) return ART_EUNSUPPORTED;     // first use under capture: nothing allocated
    // LDS for the rows a part samples (a crop never magnifies by much: the rows of a part + 3 cover every scale up to 1), two
    // workgroups per CU: at most 76 KB each
    int stage_rows = (int)std::min<int64_t>(Hh, (Hh + kLossParts - 1) / kLossParts + 4);
    if ((W & 3) != 0 || kReduceBlock % W != 0 || (int64_t)stage_rows * W * 4 > 76 * 1024) stage_rows = 0;
    const size_t stage_bytes = (size_t)stage_rows * W * sizeof(float);
    if (ws != nullptr) {
        if (moments == nullptr)
            hipLaunchKernelGGL(flux_com_parts_kernel, dim3((unsigned)P, (unsigned)B), dim3(kReduceBlock), 0, stream, flux, (int)Hh, (int)W,
                               kLossParts / P, ws);
        // (small batches - their bitmaps sit in the last-level cache - gain nothing from staged rows: 32 -> 35 us at 125 bitmaps)
        hipLaunchKernelGGL(flux_crop_pixel_loss_fwd_kernel<false>, dim3((unsigned)P, (unsigned)B), dim3(kReduceBlock), 0, stream, flux,
                           target_dims, ground_truth, (int)Hh, (int)W, (float)crop_width, (float)crop_height, kLossParts / P, ws, residual,
                           loss, centers4, center_grad_unit, moments, 0);
        hipLaunchKernelGGL(flux_crop_pixel_loss_final_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, ws, (int)B, (int)Hh,
                           (int)W, loss, centers4, center_grad_unit, moments);
    } else
    {
        if (stage_bytes > 48 * 1024) {
            static LdsGrant granted;
            const int rc = grant_dynamic_lds(reinterpret_cast<const void*>(&flux_crop_pixel_loss_fwd_kernel<true>), granted, stage_bytes);
            if (rc != ART_OK) return rc;
        }
        hipLaunchKernelGGL(flux_crop_pixel_loss_fwd_kernel<true>, dim3(1u, (unsigned)B), dim3(kReduceBlock), stage_bytes, stream, flux, target_dims,
                           ground_truth, (int)Hh, (int)W, (float)crop_width, (float)crop_height, kLossParts, (PartScratch*)nullptr, residual,
                           loss, centers4, center_grad_unit, moments, stage_rows);
    }
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_flux_crop_pixel_loss_bwd(const float* target_dims, const float* centers4, const float* grad_loss,
                                            int64_t grad_loss_stride, const float* residual, const float* center_grad_unit, int64_t B,
                                            int64_t Hh, int64_t W, double crop_width, double crop_height, float* grad_flux, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (empty_batch(B, Hh, W)) return ART_OK;
    if (!crop_args_ok(residual, target_dims, center_grad_unit, centers4, B, Hh, W) || !grad_loss || !grad_flux ||
        (grad_loss_stride != 0 && grad_loss_stride != 1))
        return ART_EINVAL;
    launch_crop_bwd_tiled<true>(stream, target_dims, centers4, center_grad_unit, residual, B, Hh, W, crop_width, crop_height, grad_flux,
                                grad_loss, grad_loss_stride);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_flux_center_of_mass(const float* flux, int64_t B, int64_t Hh, int64_t W, float* com, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (empty_batch(B, Hh, W)) return ART_OK;
    if (!crop_args_ok(flux, com, flux, com, B, Hh, W)) return ART_EINVAL;
    hipLaunchKernelGGL(flux_com_kernel<PixelWeights>, dim3((unsigned)B), dim3(kReduceBlock), 0, stream, flux, (int)Hh, (int)W, com);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_flux_center_of_mass_bwd(const float* com, const float* grad_com, int64_t B, int64_t Hh, int64_t W,
                                           float* grad_flux, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (empty_batch(B, Hh, W)) return ART_OK;
    if (!crop_args_ok(com, grad_com, grad_flux, com, B, Hh, W)) return ART_EINVAL;
    hipLaunchKernelGGL(flux_com_px_bwd_kernel, dim3((unsigned)((Hh * W + kFluxBlock - 1) / kFluxBlock), (unsigned)B), dim3(kFluxBlock),
                       0, stream, com, grad_com, (int)Hh, (int)W, grad_flux);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_flux_crop_kl_loss_fwd(const float* flux, const float* target_dims, const float* ground_truth, int64_t B,
                                         int64_t Hh, int64_t W, double crop_width, double crop_height, float* loss,
                                         float* record8, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (empty_batch(B, Hh, W)) return ART_OK;
    if (!crop_args_ok(flux, target_dims, ground_truth, loss, B, Hh, W) || !record8) return ART_EINVAL;
    hipLaunchKernelGGL(flux_crop_kl_loss_fwd_kernel, dim3((unsigned)B), dim3(kReduceBlock), 0, stream, flux, target_dims,
                       ground_truth, (int)Hh, (int)W, (float)crop_width, (float)crop_height, loss, record8);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_flux_crop_kl_loss_bwd(const float* flux, const float* target_dims, const float* ground_truth,
                                         const float* record8, const float* grad_loss, int64_t B, int64_t Hh, int64_t W,
                                         double crop_width, double crop_height, float* grad_flux, float* workspace,
                                         void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (empty_batch(B, Hh, W)) return ART_OK;
    if (!crop_args_ok(flux, target_dims, ground_truth, record8, B, Hh, W) || !grad_loss || !grad_flux || !workspace) return ART_EINVAL;
    float* grad_crop = workspace;                      // [B,Hh,W]
    float* com3 = workspace + B * Hh * W;              // [B,3]
    float* gcom = com3 + 3 * B;                        // [B,2]
    hipLaunchKernelGGL(flux_crop_kl_loss_bwd_kernel, dim3((unsigned)B), dim3(kReduceBlock), 0, stream, flux, target_dims,
                       ground_truth, record8, grad_loss, (int)Hh, (int)W, (float)crop_width, (float)crop_height, grad_crop, com3,
                       gcom);
    launch_crop_bwd_tiled<false>(stream, target_dims, com3, gcom, grad_crop, B, Hh, W, crop_width, crop_height, grad_flux);
    ART_HIP(hipGetLastError());
    return ART_OK;
}
