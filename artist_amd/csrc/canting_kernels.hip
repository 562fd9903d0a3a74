// canting_kernels.hip - art_cant_facets_fwd / _bwd (include/artist_hip_canting.h): the facet canting rotation and the
// facet translation (artist/geometry/transforms.py:276-347, artist/nurbs/surfaces.py:674-687) as an operation of their own,
// so that the canting vectors and the translations can learn.  The fused evaluation (nurbs_kernels.hip: finish_point /
// point_adjoint) treats both as constants; this file repeats its arithmetic operation by operation - the forward's bits are
// those of the fused kernel - and adds the two gradients the fused backward does not form.
//
// Backward: one workgroup per facet, a thread strides over the facet's points, writes the data gradients and keeps 13 partial
// sums in fp64 registers (the 3x3 dL/dB over points and normals together, and the four sums of the points' gradients for the
// translation).  A product of two fp32 values is exact in fp64, so only the additions round.  The sums are combined by a fixed
// shuffle tree inside a wave and in wave order across the waves (through LDS, written before it is read); one thread then
// chains dL/dB through the adjoint of canting_basis in fp64.  No atomics: a facet's bits depend on that facet alone.  A facet
// is never split over workgroups - a single heliostat is four workgroups of a few microseconds.
#include <algorithm>

#include "launch_common.hpp"

#include "../../include/artist_hip_canting.h"
#include "canting_basis.hpp"

namespace art {
namespace {

constexpr int kCantBlock = 256;
constexpr int kCantWaves = kCantBlock / 64;
constexpr int kCantFwdPointsPerBlock = 2048;      // forward: a facet's points are cut into runs of at least this many
constexpr int64_t kCantMaxDim = 2147483647LL;

// data @ R^T for one row vector (finish_point's arithmetic): out_j = ((x B[0][j] + y B[1][j]) + z B[2][j]) [+ w 0]
template <bool HOMOGENEOUS_TERM>
__device__ __forceinline__ float4 rotate_fwd(const float4 d, const float* B)
{
    float4 o;
    o.x = (d.x * B[0] + d.y * B[3]) + d.z * B[6];
    o.y = (d.x * B[1] + d.y * B[4]) + d.z * B[7];
    o.z = (d.x * B[2] + d.y * B[5]) + d.z * B[8];
    if (HOMOGENEOUS_TERM) { o.x = o.x + d.w * 0.0f; o.y = o.y + d.w * 0.0f; o.z = o.z + d.w * 0.0f; }
    o.w = d.w;
    return o;
}

// data @ R: out_k = ((x B[k][0] + y B[k][1]) + z B[k][2]) [+ w 0]
template <bool HOMOGENEOUS_TERM>
__device__ __forceinline__ float4 rotate_inv(const float4 d, const float* B)
{
    float4 o;
    o.x = (d.x * B[0] + d.y * B[1]) + d.z * B[2];
    o.y = (d.x * B[3] + d.y * B[4]) + d.z * B[5];
    o.z = (d.x * B[6] + d.y * B[7]) + d.z * B[8];
    if (HOMOGENEOUS_TERM) { o.x = o.x + d.w * 0.0f; o.y = o.y + d.w * 0.0f; o.z = o.z + d.w * 0.0f; }
    o.w = d.w;
    return o;
}

// grid = (HF, runs of points); every workgroup builds its facet's basis once (thread 0, then LDS).
__global__ __launch_bounds__(kCantBlock) void cant_facets_fwd_kernel(
    const float* __restrict__ canting, const float* __restrict__ transl, const float4* __restrict__ data_p,
    const float4* __restrict__ data_n, int inverse, int M, int per_block, float4* __restrict__ out_p, float4* __restrict__ out_n)
{
    __shared__ float s_B[9];
    const int64_t hf = blockIdx.x;
    if (threadIdx.x == 0) canting_basis(canting + hf * 8, s_B);
    __syncthreads();
    const int64_t m0 = (int64_t)blockIdx.y * per_block;
    const int64_t m1 = min((int64_t)M, m0 + per_block);
    float4 tr = make_float4(0.f, 0.f, 0.f, 0.f);
    if (transl) tr = make_float4(transl[hf * 4], transl[hf * 4 + 1], transl[hf * 4 + 2], transl[hf * 4 + 3]);
    for (int64_t m = m0 + threadIdx.x; m < m1; m += kCantBlock) {
        const int64_t i = hf * M + m;
        if (data_p) {
            float4 o = inverse ? rotate_inv<true>(data_p[i], s_B) : rotate_fwd<true>(data_p[i], s_B);
            if (transl) { o.x = o.x + tr.x; o.y = o.y + tr.y; o.z = o.z + tr.z; o.w = o.w + tr.w; }
            out_p[i] = o;
        }
        if (data_n) out_n[i] = inverse ? rotate_inv<false>(data_n[i], s_B) : rotate_fwd<false>(data_n[i], s_B);
    }
}

// 64-lane sum in a fixed tree; the result is valid in lane 0.
__device__ __forceinline__ double cant_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

struct CantBwdArgs {
    const float* canting;
    const float4 *data_p, *data_n, *g_out_p, *g_out_n;
    float4 *g_data_p, *g_data_n;
    float *g_cant, *g_tr;
    int inverse, M;
};

// One array's point: its data gradient (point_adjoint's arithmetic: g @ B, or g @ B^T for the inverse) and its nine products
// for dL/dB.  forward: out_j = sum_k data_k B[k][j] -> dB[k][j] += data_k g_j;  inverse: out_k = sum_j data_j B[k][j] ->
// dB[k][j] += g_k data_j.
__device__ __forceinline__ float4 cant_point_bwd(const float4 g, const float* B, int inverse)
{
    float4 o;
    if (inverse) {
        o.x = g.x * B[0] + g.y * B[3] + g.z * B[6];
        o.y = g.x * B[1] + g.y * B[4] + g.z * B[7];
        o.z = g.x * B[2] + g.y * B[5] + g.z * B[8];
    } else {
        o.x = g.x * B[0] + g.y * B[1] + g.z * B[2];
        o.y = g.x * B[3] + g.y * B[4] + g.z * B[5];
        o.z = g.x * B[6] + g.y * B[7] + g.z * B[8];
    }
    o.w = g.w;
    return o;
}

__device__ __forceinline__ void cant_outer(double* acc, const float4 row, const float4 col)
{
    const double r[3] = {(double)row.x, (double)row.y, (double)row.z};
    const double c[3] = {(double)col.x, (double)col.y, (double)col.z};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[3 * k + j] += r[k] * c[j];
}

// v / max(|v|, eps) backwards: g_v from g_out.  A clamped norm is a constant (clamp_min passes no gradient below its bound).
__device__ __forceinline__ void normalize_adjoint(const double* v, double eps, const double* g, double* gv)
{
    const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (n >= eps) {
        const double inv = 1.0 / n;
        const double o[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
        const double dot = (o[0] * g[0] + o[1] * g[1]) + o[2] * g[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) gv[k] = (g[k] - o[k] * dot) * inv;
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) gv[k] = g[k] / eps;
    }
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void unit3(const double* v, double eps, double* o)
{
    const double n = fmax(sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), eps);
    o[0] = v[0] / n; o[1] = v[1] / n; o[2] = v[2] / n;
}

// The adjoint of canting_basis: gB[0..2] = dL/de^, gB[3..5] = dL/dn_ortho, gB[6..8] = dL/du  ->  dL/d(e, n) as [2,4].
//   e^ = e / max(|e|, 1e-12);  u0 = e^ x n, u = u0 / max(|u0|, 1e-8);  o0 = u x e^, n_ortho = o0 / max(|o0|, 1e-8)
// backwards (c = a x b: g_a = b x g_c, g_b = g_c x a):
//   g_o0 = N'(o0) gB_o;  g_u = gB_u + e^ x g_o0;  g_e^ = gB_e + g_o0 x u
//   g_u0 = N'(u0) g_u;   g_e^ += n x g_u0;        g_n  = g_u0 x e^
//   g_e  = N'(e) g_e^
__device__ void canting_basis_adjoint(const float* cant, const double* gB, float* g_cant)
{
    const double e0[3] = {(double)cant[0], (double)cant[1], (double)cant[2]};
    const double n[3] = {(double)cant[4], (double)cant[5], (double)cant[6]};
    double e[3], u0[3], u[3], o0[3];
    unit3(e0, 1e-12, e);
    cross3(e, n, u0);
    unit3(u0, 1e-8, u);
    cross3(u, e, o0);
    double g_o0[3], g_u[3], g_e[3], g_u0[3], g_n[3], g_e0[3], t[3];
    normalize_adjoint(o0, 1e-8, gB + 3, g_o0);
    cross3(e, g_o0, t);
    g_u[0] = gB[6] + t[0]; g_u[1] = gB[7] + t[1]; g_u[2] = gB[8] + t[2];
    cross3(g_o0, u, t);
    g_e[0] = gB[0] + t[0]; g_e[1] = gB[1] + t[1]; g_e[2] = gB[2] + t[2];
    normalize_adjoint(u0, 1e-8, g_u, g_u0);
    cross3(n, g_u0, t);
    g_e[0] += t[0]; g_e[1] += t[1]; g_e[2] += t[2];
    cross3(g_u0, e, g_n);
    normalize_adjoint(e0, 1e-12, g_e, g_e0);
    g_cant[0] = (float)g_e0[0]; g_cant[1] = (float)g_e0[1]; g_cant[2] = (float)g_e0[2]; g_cant[3] = 0.0f;
    g_cant[4] = (float)g_n[0]; g_cant[5] = (float)g_n[1]; g_cant[6] = (float)g_n[2]; g_cant[7] = 0.0f;
}

__global__ __launch_bounds__(kCantBlock) void cant_facets_bwd_kernel(CantBwdArgs a)
{
    __shared__ float s_B[9];
    __shared__ double s_part[kCantWaves][13];
    const int64_t hf = blockIdx.x;
    if (threadIdx.x == 0) canting_basis(a.canting + hf * 8, s_B);
    __syncthreads();
    const bool sums = a.g_cant != nullptr;
    double acc[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) acc[k] = 0.0;
    const int64_t base = hf * a.M;
    for (int64_t m = threadIdx.x; m < a.M; m += kCantBlock) {
        const int64_t i = base + m;
        if (a.g_out_p) {
            const float4 g = a.g_out_p[i];
            if (a.g_data_p) a.g_data_p[i] = cant_point_bwd(g, s_B, a.inverse);
            if (sums) {
                const float4 d = a.data_p[i];
                if (a.inverse) cant_outer(acc, g, d); else cant_outer(acc, d, g);
            }
            if (a.g_tr) { acc[9] += (double)g.x; acc[10] += (double)g.y; acc[11] += (double)g.z; acc[12] += (double)g.w; }
        }
        if (a.g_out_n) {
            const float4 g = a.g_out_n[i];
            if (a.g_data_n) a.g_data_n[i] = cant_point_bwd(g, s_B, a.inverse);
            if (sums) {
                const float4 d = a.data_n[i];
                if (a.inverse) cant_outer(acc, g, d); else cant_outer(acc, d, g);
            }
        }
    }
    if (!sums && !a.g_tr) return;                          // (uniform: the whole workgroup leaves)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        const double s = cant_wave_sum(acc[k]);
        if (lane == 0) s_part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[13];
#pragma unroll
        for (int k = 0; k < 13; ++k) {
            double s = s_part[0][k];
#pragma unroll
            for (int w = 1; w < kCantWaves; ++w) s += s_part[w][k];
            tot[k] = s;
        }
        if (sums) canting_basis_adjoint(a.canting + hf * 8, tot, a.g_cant + hf * 8);
        if (a.g_tr) {
            float* o = a.g_tr + hf * 4;
            o[0] = (float)tot[9]; o[1] = (float)tot[10]; o[2] = (float)tot[11]; o[3] = (float)tot[12];
        }
    }
}

}  // namespace
}  // namespace art

extern "C" int art_cant_facets_fwd(const float* canting, const float* translations, const float* data_points,
                                   const float* data_normals, int inverse, int64_t HF, int64_t M, float* out_points,
                                   float* out_normals, void* stream)
{
    using namespace art;
    if (HF < 0 || M < 0 || HF > kCantMaxDim || M > kCantMaxDim) return ART_EINVAL;
    if (translations != nullptr && inverse != 0) return ART_EINVAL;
    if (HF == 0 || M == 0) return ART_OK;                          // (an empty array's pointer may well be null)
    if (canting == nullptr || (data_points == nullptr && data_normals == nullptr)) return ART_EINVAL;
    if (translations != nullptr && data_points == nullptr) return ART_EINVAL;
    if ((data_points != nullptr && out_points == nullptr) || (data_normals != nullptr && out_normals == nullptr)) return ART_EINVAL;
    // runs of points per facet: at least kCantFwdPointsPerBlock each, at most 65535 of them (gridDim.y)
    const int64_t per_block = std::max<int64_t>(kCantFwdPointsPerBlock, (M + 65534) / 65535);
    const int64_t runs = (M + per_block - 1) / per_block;
    hipLaunchKernelGGL(cant_facets_fwd_kernel, dim3((unsigned)HF, (unsigned)runs), dim3(kCantBlock), 0, (hipStream_t)stream,
                       canting, translations, reinterpret_cast<const float4*>(data_points),
                       reinterpret_cast<const float4*>(data_normals), inverse != 0 ? 1 : 0, (int)M, (int)per_block,
                       reinterpret_cast<float4*>(out_points), reinterpret_cast<float4*>(out_normals));
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_cant_facets_bwd(const float* canting, const float* data_points, const float* data_normals,
                                   const float* grad_out_points, const float* grad_out_normals, int inverse, int64_t HF,
                                   int64_t M, float* grad_data_points, float* grad_data_normals, float* grad_canting,
                                   float* grad_translations, void* stream)
{
    using namespace art;
    if (HF < 0 || M < 0 || HF > kCantMaxDim || M > kCantMaxDim) return ART_EINVAL;
    if (grad_data_points == nullptr && grad_data_normals == nullptr && grad_canting == nullptr && grad_translations == nullptr)
        return ART_EINVAL;
    if (grad_translations != nullptr && inverse != 0) return ART_EINVAL;
    if (HF == 0) return ART_OK;
    if (M == 0) {
        if (grad_canting != nullptr) ART_HIP(hipMemsetAsync(grad_canting, 0, (size_t)HF * 8 * sizeof(float), (hipStream_t)stream));
        if (grad_translations != nullptr)
            ART_HIP(hipMemsetAsync(grad_translations, 0, (size_t)HF * 4 * sizeof(float), (hipStream_t)stream));
        return ART_OK;
    }
    if (canting == nullptr) return ART_EINVAL;
    if ((grad_data_points != nullptr && grad_out_points == nullptr) || (grad_data_normals != nullptr && grad_out_normals == nullptr))
        return ART_EINVAL;
    if (grad_canting != nullptr &&
        ((grad_out_points != nullptr && data_points == nullptr) || (grad_out_normals != nullptr && data_normals == nullptr)))
        return ART_EINVAL;
    CantBwdArgs a;
    a.canting = canting;
    a.data_p = reinterpret_cast<const float4*>(data_points);
    a.data_n = reinterpret_cast<const float4*>(data_normals);
    a.g_out_p = reinterpret_cast<const float4*>(grad_out_points);
    a.g_out_n = reinterpret_cast<const float4*>(grad_out_normals);
    a.g_data_p = reinterpret_cast<float4*>(grad_data_points);
    a.g_data_n = reinterpret_cast<float4*>(grad_data_normals);
    a.g_cant = grad_canting;
    a.g_tr = grad_translations;
    a.inverse = inverse != 0 ? 1 : 0;
    a.M = (int)M;
    hipLaunchKernelGGL(cant_facets_bwd_kernel, dim3((unsigned)HF), dim3(kCantBlock), 0, (hipStream_t)stream, a);
    ART_HIP(hipGetLastError());
    return ART_OK;
}
