// regularizer_kernels.hip - art_surface_regularizers_fwd / _bwd (include/artist_hip_regularizers.h): the two surface
// regularisers that SurfaceReconstructor adds to its loss (artist/optim/regularizers.py:60-186), forward and backward, each in
// one launch over a batch of contiguous fp32 control nets [N,U,V,3].
//
// One wave per net.  The wave stages d = current - original of its net in LDS (and, in the backward, the Laplacian of d next to
// it), so every neighbour read of the clamped stencil is an LDS read.  Lane l owns the elements l, l + 64, ... of the net in that
// order and accumulates in fp64; the 64 partial sums are combined by a fixed shuffle tree.  The bits of a net therefore depend on
// that net alone - not on the launch geometry, not on N, not on the other nets - and no atomics are used.
#include "launch_common.hpp"

#include "../../include/artist_hip_regularizers.h"

namespace art {
namespace {

constexpr int kRegWave = 64;
constexpr int kRegMaxWaves = 4;                  // nets per workgroup (fewer when a net's staging is large)
constexpr int64_t kRegMaxNetFloats = 8192;       // U*V*3 per net: d (and lap) staged in LDS, at most 64 KB per workgroup
constexpr int64_t kRegMaxLdsBytes = 65536;
constexpr unsigned kRegMaxBlocks = 1u << 20;     // the workgroups stride over the nets beyond this

// The reference's Laplacian of one element with replicate padding (regularizers.py:118-129): neighbour indices clamped to the
// net, and its order of operations (((4 x - x[u-1]) - x[u+1]) - x[v-1]) - x[v+1] (the library is built with -ffp-contract=off,
// so this is torch's fp32 value bit for bit).  The clamped operator is symmetric - an edge point is its own missing neighbour,
// and the pairs (p, neighbour of p) are the same from both sides - so the same stencil is also the adjoint the backward needs.
__device__ __forceinline__ float clamped_laplacian(const float* __restrict__ x, int i, int U, int V)
{
    const int cell = i / 3;
    const int u = cell / V, v = cell - u * V;
    const int su = 3 * V;
    const float x_um = x[u > 0 ? i - su : i];
    const float x_up = x[u + 1 < U ? i + su : i];
    const float x_vm = x[v > 0 ? i - 3 : i];
    const float x_vp = x[v + 1 < V ? i + 3 : i];
    return (((4.0f * x[i] - x_um) - x_up) - x_vm) - x_vp;
}

// 64-lane sum in a fixed tree; the result is valid in lane 0.
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kRegWave);
    return v;
}

// forward: smoothness[net] = mean(lap^2), ideal[net] = mean(d^2) (either output may be null).  `waves` nets per workgroup, each
// wave owns n floats of the dynamic LDS.  The loop over groups of nets is uniform across the workgroup, so every wave reaches
// every barrier; a wave past the last net only waits.
__global__ __launch_bounds__(kRegWave * kRegMaxWaves) void surface_regularizers_fwd_kernel(
    const float* __restrict__ cur, const float* __restrict__ org, int64_t N, int U, int V, int waves,
    float* __restrict__ smoothness, float* __restrict__ ideal)
{
    extern __shared__ float reg_lds[];
    const int wave = threadIdx.x / kRegWave, lane = threadIdx.x % kRegWave;
    const int n = U * V * 3;
    float* const d = reg_lds + (size_t)wave * n;
    const int64_t groups = (N + waves - 1) / waves;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t net = g * waves + wave;
        const bool active = net < N;
        double acc_ideal = 0.0, acc_smooth = 0.0;
        if (active) {
            const float* const c = cur + net * n;
            const float* const o = org + net * n;
            for (int i = lane; i < n; i += kRegWave) {
                const float di = c[i] - o[i];
                d[i] = di;
                acc_ideal += (double)(di * di);
            }
        }
        __syncthreads();
        if (active) {
            if (smoothness != nullptr)
                for (int i = lane; i < n; i += kRegWave) {
                    const float lap = clamped_laplacian(d, i, U, V);
                    acc_smooth += (double)(lap * lap);
                }
            acc_ideal = wave_sum_f64(acc_ideal);
            acc_smooth = wave_sum_f64(acc_smooth);
            if (lane == 0) {
                if (smoothness != nullptr) smoothness[net] = (float)(acc_smooth / (double)n);
                if (ideal != nullptr) ideal[net] = (float)(acc_ideal / (double)n);
            }
        }
        __syncthreads();                          // d is overwritten by the next group
    }
}

// backward: grad_current = grad_ideal * (2/n) d + grad_smoothness * (2/n) L^T(lap), L^T = L (see clamped_laplacian); a null
// upstream gradient drops its term.  Each wave owns 2n floats of LDS (d, then lap) when the smoothness term is there, n otherwise.
__global__ __launch_bounds__(kRegWave * kRegMaxWaves) void surface_regularizers_bwd_kernel(
    const float* __restrict__ cur, const float* __restrict__ org, int64_t N, int U, int V, int waves,
    const float* __restrict__ grad_smoothness, const float* __restrict__ grad_ideal, float* __restrict__ grad_current)
{
    extern __shared__ float reg_lds[];
    const int wave = threadIdx.x / kRegWave, lane = threadIdx.x % kRegWave;
    const int n = U * V * 3;
    const bool smooth = grad_smoothness != nullptr;
    float* const d = reg_lds + (size_t)wave * (smooth ? 2 : 1) * n;
    float* const lap = d + n;
    const float two_over_n = 2.0f / (float)n;
    const int64_t groups = (N + waves - 1) / waves;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t net = g * waves + wave;
        const bool active = net < N;
        if (active) {
            const float* const c = cur + net * n;
            const float* const o = org + net * n;
            for (int i = lane; i < n; i += kRegWave) d[i] = c[i] - o[i];
        }
        __syncthreads();
        if (active && smooth)
            for (int i = lane; i < n; i += kRegWave) lap[i] = clamped_laplacian(d, i, U, V);
        __syncthreads();
        if (active) {
            const float a = grad_ideal != nullptr ? grad_ideal[net] * two_over_n : 0.0f;
            const float b = smooth ? grad_smoothness[net] * two_over_n : 0.0f;
            float* const out = grad_current + net * n;
            for (int i = lane; i < n; i += kRegWave) {
                float gi = 0.0f;
                if (grad_ideal != nullptr) gi = a * d[i];
                if (smooth) gi = gi + b * clamped_laplacian(lap, i, U, V);
                out[i] = gi;
            }
        }
        __syncthreads();
    }
}

// Launch shape from the net size alone: as many nets per workgroup (up to 4) as the LDS budget admits.
struct RegGeometry {
    int waves;
    unsigned blocks;
    size_t lds_bytes;
};

int regularizer_geometry(int64_t N, int64_t U, int64_t V, int arrays, RegGeometry* geo)
{
    if (N < 0 || U < 1 || V < 1) return ART_EINVAL;
    if (U > kRegMaxNetFloats || V > kRegMaxNetFloats || U * V * 3 > kRegMaxNetFloats) return ART_EINVAL;
    const int64_t wave_bytes = (int64_t)arrays * U * V * 3 * (int64_t)sizeof(float);
    int64_t waves = kRegMaxLdsBytes / wave_bytes;
    if (waves > kRegMaxWaves) waves = kRegMaxWaves;
    const int64_t groups = (N + waves - 1) / waves;
    geo->waves = (int)waves;
    geo->blocks = (unsigned)(groups < (int64_t)kRegMaxBlocks ? groups : (int64_t)kRegMaxBlocks);
    geo->lds_bytes = (size_t)(waves * wave_bytes);
    return ART_OK;
}

}  // namespace
}  // namespace art

extern "C" int art_surface_regularizers_fwd(const float* current, const float* original, int64_t N, int64_t U, int64_t V,
                                            float* smoothness, float* ideal, void* stream)
{
    using namespace art;
    RegGeometry geo;
    const int rc = regularizer_geometry(N, U, V, 1, &geo);
    if (rc != ART_OK) return rc;
    if (N == 0) return ART_OK;
    if (current == nullptr || original == nullptr || (smoothness == nullptr && ideal == nullptr)) return ART_EINVAL;
    hipLaunchKernelGGL(surface_regularizers_fwd_kernel, dim3(geo.blocks), dim3(kRegWave * geo.waves), geo.lds_bytes,
                       (hipStream_t)stream, current, original, N, (int)U, (int)V, geo.waves, smoothness, ideal);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_surface_regularizers_bwd(const float* current, const float* original, int64_t N, int64_t U, int64_t V,
                                            const float* grad_smoothness, const float* grad_ideal, float* grad_current,
                                            void* stream)
{
    using namespace art;
    RegGeometry geo;
    const int rc = regularizer_geometry(N, U, V, grad_smoothness != nullptr ? 2 : 1, &geo);
    if (rc != ART_OK) return rc;
    if (N == 0) return ART_OK;
    if (current == nullptr || original == nullptr || grad_current == nullptr) return ART_EINVAL;
    hipLaunchKernelGGL(surface_regularizers_bwd_kernel, dim3(geo.blocks), dim3(kRegWave * geo.waves), geo.lds_bytes,
                       (hipStream_t)stream, current, original, N, (int)U, (int)V, geo.waves, grad_smoothness, grad_ideal,
                       grad_current);
    ART_HIP(hipGetLastError());
    return ART_OK;
}
