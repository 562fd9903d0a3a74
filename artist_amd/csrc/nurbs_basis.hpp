// nurbs_basis.hpp - knot-span search and the NURBS Book's A2.3 (basis functions + first derivatives) in the reference's
// operation order, shared by nurbs_kernels.hip (evaluation) and surface_fit_kernels.hip (the fit's per-point tables).
#pragma once
#include <hip/hip_runtime.h>

#include "ray_math.hpp"      // div_noscale: n / a bit for bit, without the range scaling of the IEEE sequence

namespace art {

constexpr int kMaxDeg = 7;

// surfaces.py:198-207 (uniform) / :209-243 (search).
__device__ __forceinline__ int find_span(float x, const float* knots, int n, int deg, int uniform, int n_unique)
{
    int span;
    if (uniform) {
        span = (int)floorf(x * (float)(n_unique - 1)) + deg;
    } else {
        span = deg;
        for (int k = deg; k < n; ++k)
            if (x >= knots[k] && x < knots[k + 1]) { span = k; break; }
        const float last = knots[n];
        if (fabsf(x - last) <= 1e-5f + 1e-5f * fabsf(last)) span = n - 1;
    }
    // The reference would raise an IndexError outside [deg, n-1]; keep the LDS gathers in range.
    return min(max(span, deg), n - 1);
}

// surfaces.py:294-417 for nth_derivative = 1.  DEG > 0: compile-time degree (registers);
// DEG == 0: runtime degree `deg` (arrays may live in scratch - rare shapes only).
template <int DEG>
__device__ __forceinline__ void basis(float x, const float* knots, int span, int deg, float* N, float* D)
{
    constexpr int S = (DEG > 0 ? DEG : kMaxDeg) + 1;
    const int pdeg = DEG > 0 ? DEG : deg;
    float ndu[S][S], left[S], right[S];
    ndu[0][0] = 1.0f;
#pragma unroll
    for (int j = 1; j < S; ++j) {
        if (j > pdeg) break;
        left[j] = x - knots[span + 1 - j];
        right[j] = knots[span + j] - x;
        float saved = 0.0f;
#pragma unroll
        for (int r = 0; r < S - 1; ++r) {
            if (r >= j) break;
            ndu[j][r] = right[r + 1] + left[j - r];
            // (knot differences and basis values are far inside the normal range: div_noscale == '/')
            const float tmp = div_noscale(ndu[r][j - 1], ndu[j][r]);
            ndu[r][j] = saved + right[r + 1] * tmp;
            saved = left[j - r] * tmp;
        }
        ndu[j][j] = saved;
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
        if (j > pdeg) break;
        N[j] = ndu[j][pdeg];
    }
    const int pk = pdeg - 1;
#pragma unroll
    for (int r = 0; r < S; ++r) {
        if (r > pdeg) break;
        float d = 0.0f;
        if (r >= 1) {
            const float a0 = div_noscale(1.0f, ndu[pk + 1][r - 1]);
            d = a0 * ndu[r - 1][pk];
        }
        if (r <= pk) {
            const float a1 = div_noscale(-1.0f, ndu[pk + 1][r]);
            d += a1 * ndu[r][pk];
        }
        D[r] = d * (float)pdeg;
    }
}

__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

}  // namespace art
