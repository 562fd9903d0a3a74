// shading_kernels.hip - heliostat shading through the blocking kernels (include/artist_hip_shading.h).
//
// Shading = the sun ray to a mirror point stopped by a neighbour before it arrives.  For heliostat h with the mirror plane
// through c with unit normal n and the unit direction to the sun s = -incident (s.n != 0), the affine shear
//
//     A_h(x) = x - 2 ((x - c).n) / (s.n) * s_par,        s_par = s - (s.n) n
//
// fixes the mirror plane and maps the sunward ray p + t s of a plane point p onto the reflected ray p + t d, d = 2 (s.n) n - s,
// at the same parameter t.  The sunward ray meets a neighbour's rectangle Q at (t, u, v) exactly when the reflected ray meets
// the parallelogram A_h(Q) at the same (t, u, v): shading is blocking by per-heliostat virtual parallelograms, and the trace
// kernels (trace_kernels.hip), whose soft mask is written for parallelograms, evaluate it unchanged.  This file produces what
// they need:
//
//   cull     which rectangles can shade which heliostat (the rule below), one workgroup per heliostat, ordered ballot
//            compaction: ascending lists that do not depend on the launch
//   prims    the sheared tables (corners, spans, normals) of the listed rectangles, and their adjoint w.r.t. the real corners
//            through both paths - the shader's corners and the shaded heliostat's own plane - summed in a fixed order
//   append   the virtual rows N + h*S + k enter the candidate row of heliostat h ONLY (a virtual parallelogram of h lies in real
//            space and could sit inside another heliostat's beam: it never passes through art_blocking_filter)
//
// THE CULL RULE.  Own rectangle o = owner[h]: su = o1 - o0, sv = o3 - o0, c_h = o0 + (su + sv)/2, n_h = normalize(su x sv),
// r_h = max(|su + sv|, |su - sv|) / 2.  s = -incident[h], sn = s.n_h; |sn| < 1e-3: no shaders (the mirror receives nothing).
//     T = |s - sn n_h| / |sn|                    tangent of the incidence angle
//     g = 1 + 2 T                                bound on the norm of the inverse shear's linear part
//     kappa = g * (1.4143 * max_scatter + kShadeTilt)      largest deviation from s of a ray's preimage direction
//     r_own = 1.02 r_h + kShadeOffPlane * g      preimages of the ray origins lie within r_own of c_h
// For every rectangle j != o with centre c_j = j0 + (su_j + sv_j)/2 and rho_j = 1.06 max(|su_j + sv_j|, |su_j - sv_j|)/2 + 2e-3
// (the soft mask reaches 2.6 % of a span beyond the edges; ray_math.hpp: make_prim), w = c_j - c_h, a = w.s,
// perp = sqrt(max(|w|^2 - a^2, 0)), reach = r_own + rho_j:
//     listed  <=>  (kappa >= 0.5  or  (a >= -reach  and  perp <= reach + (a + reach) * kappa / (1 - kappa)))
//             and  (kappa >= |sn| or  sign(sn) * (w.n_h) >= -reach)
// i.e. the component along s, the 3-D distance from the sun line through c_h, and the position in front of h's plane.
// A superset of every j whose mask term can reach 1e-11 (the rejection level of ray_math.hpp's soft mask) for a ray that
// starts within 1.02 r_h of c_h and 25 mm of the plane, in a direction within 1.4143 max_scatter + kShadeTilt of d: the term
// needs a hit X' = p + t r inside the soft edge of A_h(Q_j) with t > 0, whose preimage X = A_h^-1(p) + t (s + e) lies within
// rho_j of c_j, with |A_h^-1(p) - c_h| <= r_own and |e| <= kappa.  tests/shading_ref.py restates the rule.
#include <stdint.h>

#include "launch_common.hpp"

#include "../../include/artist_hip_shading.h"

namespace art {
namespace {

constexpr int kShadeBlock = 256;
constexpr float kShadeTilt = 0.02f;        // rad: ray directions within this of the ideal reflection (local normals within 10 mrad)
constexpr float kShadeOffPlane = 0.05f;    // m: twice the largest distance of a surface point from the rectangle's plane
constexpr float kShadeMinCos = 1e-3f;      // |s.n| below this: no shaders
constexpr int64_t kShadeMaxDim = 1 << 22;

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(float f, V3 a) { return v3(f * a.x, f * a.y, f * a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ V3 load3(const float* __restrict__ p) { return v3(p[0], p[1], p[2]); }

// centre and half of the longer diagonal of rectangle k
__device__ __forceinline__ void centre_radius(const float* __restrict__ corners, int k, V3& c, float& half_diag)
{
    const float* q = corners + 16 * (int64_t)k;
    const V3 c0 = load3(q), su = load3(q + 4) - c0, sv = load3(q + 12) - c0;
    const V3 dp = su + sv, dm = su - sv;
    c = c0 + 0.5f * dp;
    half_diag = 0.5f * sqrtf(fmaxf(dot(dp, dp), dot(dm, dm)));
}

// the plane of heliostat h's own rectangle and its sun vector; ok = false: no shading for h (bad owner index, grazing sun)
struct OwnPlane { V3 c, n, s, sp; float sn, len; int o; bool ok; };

__device__ __forceinline__ OwnPlane own_plane(const float* __restrict__ corners, const int32_t* __restrict__ owner,
                                              const float* __restrict__ incident, int h, int N)
{
    OwnPlane p;
    p.o = owner[h];
    p.ok = (unsigned)p.o < (unsigned)N;
    const float* q = corners + 16 * (int64_t)(p.ok ? p.o : 0);
    const V3 c0 = load3(q), su = load3(q + 4) - c0, sv = load3(q + 12) - c0;
    p.c = c0 + 0.5f * (su + sv);
    const V3 m = cross(su, sv);
    p.len = fmaxf(sqrtf(dot(m, m)), 1e-12f);               // torch.nn.functional.normalize
    p.n = (1.0f / p.len) * m;
    p.s = v3(-incident[4 * (int64_t)h], -incident[4 * (int64_t)h + 1], -incident[4 * (int64_t)h + 2]);
    p.sn = dot(p.s, p.n);
    p.sp = p.s - p.sn * p.n;
    p.ok = p.ok && fabsf(p.sn) >= kShadeMinCos;
    return p;
}

__global__ __launch_bounds__(kShadeBlock) void shading_cull_kernel(const float* __restrict__ corners, const int32_t* __restrict__ owner,
                                                                   const float* __restrict__ incident, int N, float max_scatter,
                                                                   int S, int32_t* __restrict__ shader_idx,
                                                                   int32_t* __restrict__ shade_count)
{
    __shared__ int s_wave[kShadeBlock / 64];
    const int h = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < S; k += kShadeBlock) shader_idx[(int64_t)h * S + k] = -1;
    const OwnPlane own = own_plane(corners, owner, incident, h, N);
    if (!own.ok) {                                          // (workgroup-uniform)
        if (threadIdx.x == 0) shade_count[h] = 0;
        return;
    }
    __syncthreads();                                        // the -1s are written before any slot is
    V3 ch; float rh;
    centre_radius(corners, own.o, ch, rh);
    const float asn = fabsf(own.sn);
    const float T = sqrtf(dot(own.sp, own.sp)) / asn;
    const float g = 1.0f + 2.0f * T;
    const float kappa = g * (1.4143f * max_scatter + kShadeTilt);
    const float r_own = 1.02f * rh + kShadeOffPlane * g;
    const float sgn = own.sn > 0.0f ? 1.0f : -1.0f;
    int base = 0;
    for (int k0 = 0; k0 < N; k0 += kShadeBlock) {
        const int j = k0 + (int)threadIdx.x;
        bool listed = false;
        if (j < N && j != own.o) {
            V3 cj; float rj;
            centre_radius(corners, j, cj, rj);
            const float reach = r_own + (1.06f * rj + 2e-3f);
            const V3 w = cj - ch;
            const float a = dot(w, own.s);
            const float perp = sqrtf(fmaxf(dot(w, w) - a * a, 0.0f));
            const bool along = kappa >= 0.5f || (a >= -reach && perp <= reach + (a + reach) * (kappa / (1.0f - kappa)));
            const bool front = kappa >= asn || sgn * dot(w, own.n) >= -reach;
            listed = along && front;
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(listed);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = base;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (listed) {
            const int slot = before + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < S) shader_idx[(int64_t)h * S + slot] = j;
        }
        for (int w = 0; w < kShadeBlock / 64; ++w) base += s_wave[w];
        __syncthreads();
    }
    if (threadIdx.x == 0) shade_count[h] = base;
}

// one thread per slot (h, k): the sheared corners of rectangle shader_idx[h][k], the spans and the normal formed from them
__global__ __launch_bounds__(kShadeBlock) void shading_prims_fwd_kernel(const float* __restrict__ corners, const int32_t* __restrict__ owner,
                                                                        const float* __restrict__ incident,
                                                                        const int32_t* __restrict__ shader_idx, int H, int N, int S,
                                                                        float4* __restrict__ out_corners, float4* __restrict__ out_spans,
                                                                        float4* __restrict__ out_normals)
{
    const int64_t i = (int64_t)blockIdx.x * kShadeBlock + threadIdx.x;
    if (i >= (int64_t)H * S) return;
    const int h = (int)(i / S);
    const int j = shader_idx[i];
    const OwnPlane own = own_plane(corners, owner, incident, h, N);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!own.ok || (unsigned)j >= (unsigned)N) {
        for (int c = 0; c < 4; ++c) out_corners[4 * i + c] = zero;
        out_spans[2 * i] = zero; out_spans[2 * i + 1] = zero;
        out_normals[i] = zero;
        return;
    }
    const float* q = corners + 16 * (int64_t)j;
    V3 y[4]; float w[4];
    for (int c = 0; c < 4; ++c) {
        const V3 x = load3(q + 4 * c);
        const float a = dot(x - own.c, own.n) / own.sn;
        y[c] = x - (2.0f * a) * own.sp;
        w[c] = q[4 * c + 3];
        out_corners[4 * i + c] = make_float4(y[c].x, y[c].y, y[c].z, w[c]);
    }
    const V3 U = y[1] - y[0], V = y[3] - y[0];
    out_spans[2 * i] = make_float4(U.x, U.y, U.z, w[1] - w[0]);
    out_spans[2 * i + 1] = make_float4(V.x, V.y, V.z, w[3] - w[0]);
    const V3 M = cross(U, V);
    const float il = 1.0f / fmaxf(sqrtf(dot(M, M)), 1e-12f);
    out_normals[i] = make_float4(M.x * il, M.y * il, M.z * il, 0.0f);
}

// Adjoint, first pass: one thread per slot.  scratch[i] = 12 floats for the corners of the SHADER (4 x xyz) and 12 for the
// corners of the heliostat's OWN rectangle (through c_h and n_h); an empty slot leaves 24 zeros.
__global__ __launch_bounds__(kShadeBlock) void shading_prims_bwd_slot_kernel(const float* __restrict__ corners, const int32_t* __restrict__ owner,
                                                                             const float* __restrict__ incident,
                                                                             const int32_t* __restrict__ shader_idx,
                                                                             const float* __restrict__ g_corners, const float* __restrict__ g_spans,
                                                                             const float* __restrict__ g_normals, int H, int N, int S,
                                                                             float* __restrict__ scratch)
{
    const int64_t i = (int64_t)blockIdx.x * kShadeBlock + threadIdx.x;
    if (i >= (int64_t)H * S) return;
    const int h = (int)(i / S);
    const int j = shader_idx[i];
    float* __restrict__ out = scratch + 24 * i;
    const OwnPlane own = own_plane(corners, owner, incident, h, N);
    if (!own.ok || (unsigned)j >= (unsigned)N) {
        for (int c = 0; c < 24; ++c) out[c] = 0.0f;
        return;
    }
    // the forward again
    const float* q = corners + 16 * (int64_t)j;
    V3 x[4], y[4]; float a[4];
    for (int c = 0; c < 4; ++c) {
        x[c] = load3(q + 4 * c);
        a[c] = dot(x[c] - own.c, own.n) / own.sn;
        y[c] = x[c] - (2.0f * a[c]) * own.sp;
    }
    const V3 U = y[1] - y[0], V = y[3] - y[0];
    const V3 M = cross(U, V);
    const float lenM = sqrtf(dot(M, M));
    // normal -> M -> spans -> sheared corners
    V3 gY[4];
    for (int c = 0; c < 4; ++c) gY[c] = load3(g_corners + 16 * i + 4 * c);
    V3 gU = load3(g_spans + 8 * i), gV = load3(g_spans + 8 * i + 4);
    if (lenM > 1e-12f) {                                   // (a clamped norm passes the gradient of a plain scaling)
        const V3 nv = (1.0f / lenM) * M, gN = load3(g_normals + 4 * i);
        const V3 gM = (1.0f / lenM) * (gN - dot(nv, gN) * nv);
        gU = gU + cross(V, gM);
        gV = gV + cross(gM, U);
    } else {
        const V3 gM = 1e12f * load3(g_normals + 4 * i);
        gU = gU + cross(V, gM);
        gV = gV + cross(gM, U);
    }
    gY[1] = gY[1] + gU; gY[3] = gY[3] + gV; gY[0] = gY[0] - (gU + gV);
    // y_c = x_c - 2 a_c sp,  a_c = ((x_c - c).n) / sn
    V3 gc = v3(0.f, 0.f, 0.f), gn = v3(0.f, 0.f, 0.f), gsp = v3(0.f, 0.f, 0.f);
    float gsn = 0.0f;
    const float isn = 1.0f / own.sn;
    for (int c = 0; c < 4; ++c) {
        const float ga = -2.0f * dot(gY[c], own.sp);
        const V3 gx = gY[c] + (ga * isn) * own.n;
        out[3 * c] = gx.x; out[3 * c + 1] = gx.y; out[3 * c + 2] = gx.z;
        gc = gc - (ga * isn) * own.n;
        gn = gn + (ga * isn) * (x[c] - own.c);
        gsn = gsn - ga * a[c] * isn;
        gsp = gsp - (2.0f * a[c]) * gY[c];
    }
    // sp = s - sn n,  sn = s.n
    gsn = gsn - dot(gsp, own.n);
    gn = gn - own.sn * gsp;
    gn = gn + gsn * own.s;
    // n = m / max(|m|, 1e-12),  m = su x sv,  c = o0 + (su + sv)/2
    const float* qo = corners + 16 * (int64_t)own.o;
    const V3 o0 = load3(qo), su = load3(qo + 4) - o0, sv = load3(qo + 12) - o0;
    const V3 gm = own.len > 1e-12f ? (1.0f / own.len) * (gn - dot(own.n, gn) * own.n) : 1e12f * gn;
    const V3 gsu = cross(sv, gm) + 0.5f * gc, gsv = cross(gm, su) + 0.5f * gc;
    const V3 g0 = gc - (gsu + gsv);
    out[12] = g0.x; out[13] = g0.y; out[14] = g0.z;
    out[15] = gsu.x; out[16] = gsu.y; out[17] = gsu.z;
    out[18] = 0.0f; out[19] = 0.0f; out[20] = 0.0f;
    out[21] = gsv.x; out[22] = gsv.y; out[23] = gsv.z;
}

// Adjoint, second pass: one workgroup per real rectangle j.  Thread t adds, in slot order, the slots i = t, t + 256, ... that
// name j as their shader or whose heliostat owns j; the 256 partial sums are added by a fixed tree.  Every row is written.
__global__ __launch_bounds__(kShadeBlock) void shading_prims_bwd_sum_kernel(const int32_t* __restrict__ owner, const int32_t* __restrict__ shader_idx,
                                                                            const float* __restrict__ scratch, int H, int N, int S,
                                                                            float* __restrict__ g_prim_corners)
{
    __shared__ float s_part[kShadeBlock][13];
    const int j = blockIdx.x, tid = threadIdx.x;
    float acc[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) acc[c] = 0.0f;
    const int64_t slots = (int64_t)H * S;
    for (int64_t i = tid; i < slots; i += kShadeBlock) {
        if (shader_idx[i] < 0) continue;                   // (empty slots hold zeros: skipped for speed only)
        const float* __restrict__ v = scratch + 24 * i;
        if (shader_idx[i] == j)
#pragma unroll
            for (int c = 0; c < 12; ++c) acc[c] += v[c];
        if (owner[i / S] == j)
#pragma unroll
            for (int c = 0; c < 12; ++c) acc[c] += v[12 + c];
    }
#pragma unroll
    for (int c = 0; c < 12; ++c) s_part[tid][c] = acc[c];
    __syncthreads();
    for (int half = kShadeBlock / 2; half > 0; half >>= 1) {
        if (tid < half)
#pragma unroll
            for (int c = 0; c < 12; ++c) s_part[tid][c] += s_part[tid + half][c];
        __syncthreads();
    }
    if (tid < 16) g_prim_corners[16 * (int64_t)j + tid] = (tid & 3) < 3 ? s_part[0][3 * (tid >> 2) + (tid & 3)] : 0.0f;
}

__global__ __launch_bounds__(kShadeBlock) void shading_append_kernel(const int32_t* __restrict__ shader_idx, const int32_t* __restrict__ shade_count,
                                                                     int H, int N, int S, int Cmax, int32_t* __restrict__ cand,
                                                                     int32_t* __restrict__ cand_count)
{
    const int h = blockIdx.x * kShadeBlock + threadIdx.x;
    if (h >= H) return;
    const int listed = cand_count[h];
    if (listed > Cmax) return;                             // the filter's own overflow: the row is full, the count says so
    int32_t* __restrict__ row = cand + (int64_t)h * Cmax;
    const int found = shade_count[h];
    const int n = min(max(found, 0), S);
    int at = max(listed, 0), last = -1;
    bool overflow = found > S;
    for (int k = 0; k < n; ++k) {
        if (shader_idx[(int64_t)h * S + k] < 0) continue;
        last = N + h * S + k;
        if (at < Cmax) row[at++] = last; else overflow = true;
    }
    if (overflow) {
        // the trace kernels read all Cmax entries of an overflowed row before they poison the heliostat: every entry is valid
        // (a count beyond S with no slot filled - no list of art_shading_cull - is reported all the same: a row of h's own)
        if (last < 0) last = N + h * S;
        for (; at < Cmax; ++at) row[at] = last;
        cand_count[h] = Cmax + 1;
    } else {
        cand_count[h] = at;
    }
}

bool bad_dims(int64_t H, int64_t N, int64_t S)
{
    return H < 0 || N < 0 || S < 1 || H > kShadeMaxDim || N > kShadeMaxDim || S > 4096 || H * S > kShadeMaxDim ||
           N + H * S > 2147483647LL / 16;
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kShadeBlock - 1) / kShadeBlock); }

}  // namespace
}  // namespace art

using namespace art;

extern "C" int art_shading_cull(const float* prim_corners, const int32_t* owner, const float* incident, int64_t H, int64_t N,
                                double max_scatter_angle, int64_t S, int32_t* shader_idx, int32_t* shade_count, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_dims(H, N, S) || !(max_scatter_angle >= 0.0) || max_scatter_angle > 10.0) return ART_EINVAL;
    if (H == 0) return ART_OK;
    if (!owner || !incident || !shader_idx || !shade_count || (N > 0 && !prim_corners)) return ART_EINVAL;
    if (N == 0) {                                           // nothing can shade: empty lists, no launch
        ART_HIP(hipMemsetAsync(shader_idx, 0xFF, sizeof(int32_t) * H * S, stream));
        ART_HIP(hipMemsetAsync(shade_count, 0, sizeof(int32_t) * H, stream));
        return ART_OK;
    }
    hipLaunchKernelGGL(shading_cull_kernel, dim3((unsigned)H), dim3(kShadeBlock), 0, stream, prim_corners, owner, incident, (int)N,
                       (float)max_scatter_angle, (int)S, shader_idx, shade_count);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_shading_prims_fwd(const float* prim_corners, const int32_t* owner, const float* incident, const int32_t* shader_idx,
                                     int64_t H, int64_t N, int64_t S, float* shade_corners, float* shade_spans, float* shade_normals,
                                     void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_dims(H, N, S)) return ART_EINVAL;
    if (H == 0) return ART_OK;
    if (!owner || !incident || !shader_idx || !shade_corners || !shade_spans || !shade_normals || (N > 0 && !prim_corners))
        return ART_EINVAL;
    if ((reinterpret_cast<uintptr_t>(shade_corners) | reinterpret_cast<uintptr_t>(shade_spans) |
         reinterpret_cast<uintptr_t>(shade_normals)) % 16 != 0) return ART_EINVAL;
    hipLaunchKernelGGL(shading_prims_fwd_kernel, dim3(blocks_for(H * S)), dim3(kShadeBlock), 0, stream, prim_corners, owner, incident,
                       shader_idx, (int)H, (int)N, (int)S, reinterpret_cast<float4*>(shade_corners),
                       reinterpret_cast<float4*>(shade_spans), reinterpret_cast<float4*>(shade_normals));
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_shading_prims_bwd(const float* prim_corners, const int32_t* owner, const float* incident, const int32_t* shader_idx,
                                     const float* grad_shade_corners, const float* grad_shade_spans, const float* grad_shade_normals,
                                     int64_t H, int64_t N, int64_t S, float* scratch, float* grad_prim_corners, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_dims(H, N, S)) return ART_EINVAL;
    if (N == 0) return ART_OK;
    if (!grad_prim_corners) return ART_EINVAL;
    if (H == 0) {                                           // no slot contributes: the gradient is written all the same
        ART_HIP(hipMemsetAsync(grad_prim_corners, 0, sizeof(float) * 16 * N, stream));
        return ART_OK;
    }
    if (!prim_corners || !owner || !incident || !shader_idx || !grad_shade_corners || !grad_shade_spans || !grad_shade_normals ||
        !scratch) return ART_EINVAL;
    hipLaunchKernelGGL(shading_prims_bwd_slot_kernel, dim3(blocks_for(H * S)), dim3(kShadeBlock), 0, stream, prim_corners, owner,
                       incident, shader_idx, grad_shade_corners, grad_shade_spans, grad_shade_normals, (int)H, (int)N, (int)S, scratch);
    hipLaunchKernelGGL(shading_prims_bwd_sum_kernel, dim3((unsigned)N), dim3(kShadeBlock), 0, stream, owner, shader_idx, scratch,
                       (int)H, (int)N, (int)S, grad_prim_corners);
    ART_HIP(hipGetLastError());
    return ART_OK;
}

extern "C" int art_shading_append(const int32_t* shader_idx, const int32_t* shade_count, int64_t H, int64_t N, int64_t S, int64_t Cmax,
                                  int32_t* cand, int32_t* cand_count, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_dims(H, N, S) || Cmax < 1 || Cmax > kShadeMaxDim) return ART_EINVAL;
    if (H == 0) return ART_OK;
    if (!shader_idx || !shade_count || !cand || !cand_count) return ART_EINVAL;
    hipLaunchKernelGGL(shading_append_kernel, dim3(blocks_for(H)), dim3(kShadeBlock), 0, stream, shader_idx, shade_count, (int)H, (int)N,
                       (int)S, (int)Cmax, cand, cand_count);
    ART_HIP(hipGetLastError());
    return ART_OK;
}
