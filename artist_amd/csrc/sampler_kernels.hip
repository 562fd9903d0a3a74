// sampler_kernels.hip - art_sample_distortions and art_sample_radial_distortions (include/artist_hip_sampler.h):
// the sun-shape distortion sample of a light source, rows of [H,R,P] (u, e) pairs
// written as one interleaved [n_rows,R,P,2] buffer in one launch.
//
// Counter-based: pair j of heliostat row `row` is Philox4x32-10(counter (j, row), key seed) followed by the shape's rule
// (Box-Muller for the Gaussian, a quantile-table lookup for a radial shape), so every output bit is a function of
// (seed, row, R, P, law or table) alone.  Stores only: 16 B per lane per pair.
#include "launch_common.hpp"

#include "../../include/artist_hip_sampler.h"

namespace art {
namespace {

constexpr int kSamplerThreads = 256;
constexpr int64_t kMaxRadialIntervals = 4096;                                // K pairs of 8 B: 32 KiB of LDS at the most
constexpr unsigned kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;       // Random123 philox4x32 multipliers
constexpr unsigned kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;       // ... and Weyl key increments

// Philox4x32-10 (Random123): ten rounds, the key bumped between rounds.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        if (round > 0) {
            k0 += kPhiloxW0;
            k1 += kPhiloxW1;
        }
        const unsigned hi0 = __umulhi(kPhiloxM0, c.x), lo0 = kPhiloxM0 * c.x;
        const unsigned hi1 = __umulhi(kPhiloxM1, c.z), lo1 = kPhiloxM1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    }
    return c;
}

struct Law {
    float loc_u, loc_e, l00, l10, l11;
};

// Box-Muller of one 32-bit pair, then loc + scale_tril @ z.  a = x_even 2^-32 + 2^-33 lies in (0, 1] (never 0: no
// infinite radius); the hardware log is base 2 and the hardware sin / cos take revolutions, so b goes in as it is.
__device__ __forceinline__ float2 gaussian_pair(unsigned x_even, unsigned x_odd, const Law& law)
{
    const float a = (float)x_even * 0x1p-32f + 0x1p-33f;
    const float b = (float)x_odd * 0x1p-32f;
    const float rho = __builtin_amdgcn_sqrtf(__builtin_amdgcn_logf(a) * -1.38629436111989061883f);   // -2 ln a = -2 ln2 log2 a
    const float z0 = rho * __builtin_amdgcn_cosf(b);
    const float z1 = rho * __builtin_amdgcn_sinf(b);
    return make_float2(law.loc_u + law.l00 * z0, law.loc_e + (law.l10 * z0 + law.l11 * z1));
}

// A shape turns the 32-bit pair of one ray into its (u, e): stage() runs once per workgroup before the first ray.
struct GaussianShape {
    Law law;
    __device__ __forceinline__ void stage(float2*) const {}
    __device__ __forceinline__ float2 operator()(unsigned x_even, unsigned x_odd, const float2*) const
    {
        return gaussian_pair(x_even, x_odd, law);
    }
};

// A radially symmetric shape as K annuli of equal energy: table[k] is the squared radius below which k/K of the energy
// lies, and theta^2 is linear in the quantile between two nodes.  The workgroup keeps the table in LDS as K pairs
// (table[i], table[i+1] - table[i]): the lookup is one 8-byte read at a random index (ds_read_b64: 64 banks, conflicts only
// inside a 32-lane half; equal indices broadcast, so K = 1 costs one cycle).  All K pairs are written, and the barrier
// passed, before any lane reads one: nothing of the LDS a workgroup inherits is ever read.
struct RadialShape {
    float loc_u, loc_e;
    const float* __restrict__ table;   // [K+1], device
    int K;
    __device__ __forceinline__ void stage(float2* nodes) const
    {
        for (int i = threadIdx.x; i < K; i += kSamplerThreads) {
            const float lo = table[i];
            nodes[i] = make_float2(lo, table[i + 1] - lo);
        }
        __syncthreads();
    }
    // q = x_even 2^-32 + 2^-33 in (0, 1] is the quantile, b = x_odd 2^-32 the azimuth in revolutions.  t = qK <= K, so
    // i = min((int)t, K-1) lies in [0, K-1] and f = t - i in [0, 1].
    __device__ __forceinline__ float2 operator()(unsigned x_even, unsigned x_odd, const float2* nodes) const
    {
        const float q = (float)x_even * 0x1p-32f + 0x1p-33f;
        const float b = (float)x_odd * 0x1p-32f;
        const float t = q * (float)K;
        const int i = min((int)t, K - 1);
        const float f = t - (float)i;
        const float2 node = nodes[i];
        const float theta = __builtin_amdgcn_sqrtf(node.x + f * node.y);
        return make_float2(loc_u + theta * __builtin_amdgcn_cosf(b), loc_e + theta * __builtin_amdgcn_sinf(b));
    }
};

// grid.y strides over the rows, grid.x * blockDim.x over the pairs of a row.  VEC4: R*P even and `out` 16-byte
// aligned, so every pair is one aligned float4; otherwise each ray is one float2 (a row may start 8 bytes into a line).
template <bool VEC4, class Shape>
__global__ __launch_bounds__(kSamplerThreads) void sample_distortions_kernel(
    unsigned key0, unsigned key1, const int64_t* __restrict__ rows, int64_t n_rows, int64_t rays_per_row, Shape shape,
    float* __restrict__ out)
{
    extern __shared__ float2 staged[];                                 // RadialShape: K pairs; GaussianShape: none
    shape.stage(staged);
    const int64_t n_pairs = (rays_per_row + 1) >> 1;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = blockIdx.y; k < n_rows; k += gridDim.y) {
        const uint64_t row = (uint64_t)rows[k];
        float* const row_out = out + k * rays_per_row * 2;
        for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_pairs; j += stride) {
            const uint4 x = philox4x32_10(make_uint4((unsigned)j, (unsigned)((uint64_t)j >> 32), (unsigned)row,
                                                     (unsigned)(row >> 32)), key0, key1);
            const float2 g0 = shape(x.x, x.y, staged);
            const float2 g1 = shape(x.z, x.w, staged);
            if (VEC4) {
                reinterpret_cast<float4*>(row_out)[j] = make_float4(g0.x, g0.y, g1.x, g1.y);
            } else {
                reinterpret_cast<float2*>(row_out)[2 * j] = g0;
                if (2 * j + 1 < rays_per_row) reinterpret_cast<float2*>(row_out)[2 * j + 1] = g1;
            }
        }
    }
}

// The checks and the launch that both entry points share.  `lds_bytes`: what the shape stages per workgroup.
template <class Shape>
int sample_rows(int64_t seed, const int64_t* rows, int64_t n_rows, int64_t R, int64_t P, const Shape& shape, bool shape_ok,
                size_t lds_bytes, float* out, void* stream)
{
    if (n_rows < 0 || R < 0 || P < 0) return ART_EINVAL;
    if (n_rows == 0 || R == 0 || P == 0) return ART_OK;
    if (rows == nullptr || out == nullptr || !shape_ok || ((uintptr_t)out & 7) != 0) return ART_EINVAL;
    if (R > INT64_MAX / P || R * P > INT64_MAX / 2 / n_rows) return ART_EINVAL;   // element offsets must fit int64
    const int64_t rays = R * P;
    const int64_t n_pairs = (rays + 1) >> 1;
    const uint64_t key = (uint64_t)seed;
    // ~32 workgroups per CU in all, each lane looping over pairs (a lane per pair would be ~2e6 workgroups at the metric field)
    const unsigned gy = (unsigned)(n_rows < 65535 ? n_rows : 65535);
    const int64_t gx_need = (n_pairs + kSamplerThreads - 1) / kSamplerThreads;
    int64_t gx = (8192 + gy - 1) / gy;
    if (gx > gx_need) gx = gx_need;
    const dim3 grid((unsigned)gx, gy);
    hipStream_t s = (hipStream_t)stream;
    if ((rays & 1) == 0 && ((uintptr_t)out & 15) == 0)
        hipLaunchKernelGGL((sample_distortions_kernel<true, Shape>), grid, dim3(kSamplerThreads), lds_bytes, s, (unsigned)key,
                           (unsigned)(key >> 32), rows, n_rows, rays, shape, out);
    else
        hipLaunchKernelGGL((sample_distortions_kernel<false, Shape>), grid, dim3(kSamplerThreads), lds_bytes, s, (unsigned)key,
                           (unsigned)(key >> 32), rows, n_rows, rays, shape, out);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

}  // namespace
}  // namespace art

extern "C" int art_sample_distortions(int64_t seed, const int64_t* rows, int64_t n_rows, int64_t R, int64_t P, float loc_u,
                                      float loc_e, float l00, float l10, float l11, float* out, void* stream)
{
    using namespace art;
    return sample_rows(seed, rows, n_rows, R, P, GaussianShape{Law{loc_u, loc_e, l00, l10, l11}}, true, 0, out, stream);
}

extern "C" int art_sample_radial_distortions(int64_t seed, const int64_t* rows, int64_t n_rows, int64_t R, int64_t P, float loc_u,
                                             float loc_e, const float* table, int64_t K, float* out, void* stream)
{
    using namespace art;
    if (K < 1 || K > kMaxRadialIntervals) return ART_EINVAL;
    return sample_rows(seed, rows, n_rows, R, P, RadialShape{loc_u, loc_e, table, (int)K}, table != nullptr,
                       (size_t)K * sizeof(float2), out, stream);
}

