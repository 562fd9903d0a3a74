// launch_common.hpp - error plumbing + small wave-level helpers shared by the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>

#include "../../include/artist_hip.h"

namespace art {

// hipError_t of the last failing HIP call on this thread (art_last_hip_error()).
extern thread_local int g_last_hip_error;

#define ART_HIP(expr)                                   \
    do {                                                \
        hipError_t err__ = (expr);                      \
        if (err__ != hipSuccess) {                      \
            art::g_last_hip_error = (int)err__;         \
            return ART_ELAUNCH;                         \
        }                                               \
    } while (0)

// Graph capture (include/artist_hip.h, Conventions): state that the library creates on first use - an allocation, a stream, an
// event - is never created while the calling stream is being captured: an allocation made then fails AND invalidates the
// capture.  Every such site asks this BEFORE it creates anything and, when the answer is yes, creates nothing; its entry point
// returns ART_EUNSUPPORTED without having made a HIP call that could fail, so the capture stays valid.  Asked on the creating
// path only: a call that finds its state pays nothing.
static inline bool stream_is_capturing(hipStream_t stream)
{
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    const hipError_t rc = hipStreamIsCapturing(stream, &status);
    if (rc != hipSuccess) {
        (void)hipGetLastError();
        return rc == hipErrorStreamCaptureImplicit;     // the legacy stream while a blocking stream captures: create nothing either
    }
    return status != hipStreamCaptureStatusNone;
}
// The return code of an entry point whose first-use state (status word, work counters, window tables, side stream, part scratch)
// could not be had: ART_EUNSUPPORTED when `stream` is being captured - nothing was created, no HIP call has failed, and the
// caller runs the step once outside a capture first -, else the allocation failed.
static inline int first_use_error(hipStream_t stream)
{
    if (stream_is_capturing(stream)) return ART_EUNSUPPORTED;
    g_last_hip_error = (int)hipErrorOutOfMemory;
    return ART_ELAUNCH;
}

// The dynamic-LDS limit of a kernel (hipFuncAttributeMaxDynamicSharedMemorySize) is an attribute of the function on a GPU, not
// of a launch: it is raised when a launch asks for more than any launch of that kernel before it on this GPU, and left alone
// otherwise - so a launch that repeats an earlier one (every launch of a captured step after its warm-up) makes no call besides
// the launch itself.  `granted` is the caller's, one zero-initialised array per kernel instantiation.
constexpr int kLdsGrantDevices = 64;
struct LdsGrant { std::atomic<int> bytes[kLdsGrantDevices]; std::mutex lock; };
static inline int grant_dynamic_lds(const void* kernel, LdsGrant& granted, size_t lds)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kLdsGrantDevices) {
        ART_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        return ART_OK;
    }
    if ((int)lds <= granted.bytes[dev].load(std::memory_order_acquire)) return ART_OK;
    std::lock_guard<std::mutex> guard(granted.lock);
    if ((int)lds <= granted.bytes[dev].load(std::memory_order_relaxed)) return ART_OK;
    ART_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    granted.bytes[dev].store((int)lds, std::memory_order_release);
    return ART_OK;
}

// Diagnostic knobs (launch geometry, A/B paths; results are the same bits or within the documented rounding for every value):
// the library reads ARTIST_HIP_* variables ONLY when ARTIST_HIP_DEBUG=1 is set - a caller's environment cannot change what the
// product launches (tests and tools/ set both).
static inline const char* debug_env_str(const char* name)       // nullptr unless ARTIST_HIP_DEBUG=1 and the variable is set
{
    const char* dbg = getenv("ARTIST_HIP_DEBUG");
    if (dbg == nullptr || dbg[0] != '1') return nullptr;
    return getenv(name);
}
static inline int debug_env_int(const char* name, int dflt)
{
    const char* v = debug_env_str(name);
    return (v && *v) ? atoi(v) : dflt;
}

// 64-lane wave sum (gfx950 wavefront = 64); result valid in lane 0.
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_sum_f32(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// out_j = sum_k x_k M[j][k], k sequential (row vector times M^T)
__device__ __forceinline__ float4 apply_mt(const float4 x, const float* __restrict__ M)
{
    float4 o;
    o.x = ((x.x * M[0] + x.y * M[1]) + x.z * M[2]) + x.w * M[3];
    o.y = ((x.x * M[4] + x.y * M[5]) + x.z * M[6]) + x.w * M[7];
    o.z = ((x.x * M[8] + x.y * M[9]) + x.z * M[10]) + x.w * M[11];
    o.w = ((x.x * M[12] + x.y * M[13]) + x.z * M[14]) + x.w * M[15];
    return o;
}

// g_x_k = sum_j g_j M[j][k]
__device__ __forceinline__ float4 apply_m(const float4 g, const float* __restrict__ M)
{
    float4 o;
    o.x = ((g.x * M[0] + g.y * M[4]) + g.z * M[8]) + g.w * M[12];
    o.y = ((g.x * M[1] + g.y * M[5]) + g.z * M[9]) + g.w * M[13];
    o.z = ((g.x * M[2] + g.y * M[6]) + g.z * M[10]) + g.w * M[14];
    o.w = ((g.x * M[3] + g.y * M[7]) + g.z * M[11]) + g.w * M[15];
    return o;
}

}  // namespace art
