// Diagnostic hooks of the trace kernels - the ONLY preprocessor conditionals on ART_* macros in this directory.
//
// The product build defines no switch: every kNo* / kCountStrays below is a constexpr false, Timeline is an empty struct whose
// members are empty inline functions, and the two host dumps are empty too - the device code is the one without this header.
// A diagnostic library is the same sources built with -D flags (make DIAG="-DART_..." OBJDIR=... OUT=..., see the Makefile and
// tools/diag/README.md):
//   ART_DEBUG_TIMELINE          every work item records its phase time stamps in g_timeline; art_trace_fwd / art_trace_bwd write
//                               the last call's records to $ART_TIMELINE_OUT / $ART_TIMELINE_OUT_BWD (tools/timeline.sh).
//                               Results are unchanged.
//   ART_DEBUG_COUNT_STRAYS      generic forward item: factors row 2 = share of stray rays (tools/stray_stats.py)
//   ART_ABLATE_NO_LDS_ATOMICS   forward items: operands kept alive, no LDS adds
//   ART_ABLATE_NO_STRAYS        no stray-ray blocks, forward and backward
//   ART_ABLATE_NO_LOADS         distortion angles synthesised in registers, no HBM stream
//   ART_ABLATE_NO_FLUSH         the flush of the window keeps its loop and drops its global atomics
// The ART_ABLATE_* and ART_DEBUG_COUNT_STRAYS builds compute WRONG results on purpose, to price a stage (tools/ablate.sh).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#if defined(ART_DEBUG_TIMELINE) && defined(ART_TIMELINE_RECORDS_HERE)
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#endif

namespace art {
namespace diag {

#ifdef ART_ABLATE_NO_LDS_ATOMICS
constexpr bool kNoLdsAtomics = true;
#else
constexpr bool kNoLdsAtomics = false;
#endif
#ifdef ART_ABLATE_NO_STRAYS
constexpr bool kNoStrays = true;
#else
constexpr bool kNoStrays = false;
#endif
#ifdef ART_ABLATE_NO_LOADS
constexpr bool kNoLoads = true;
#else
constexpr bool kNoLoads = false;
#endif
#ifdef ART_ABLATE_NO_FLUSH
constexpr bool kNoFlush = true;
#else
constexpr bool kNoFlush = false;
#endif
#ifdef ART_DEBUG_COUNT_STRAYS
constexpr bool kCountStrays = true;
#else
constexpr bool kCountStrays = false;
#endif

// (only in the translation unit of the trace kernels, which defines ART_TIMELINE_RECORDS_HERE before it includes this header:
//  any other unit that includes it gets the empty hooks and no copy of the 1 MB record array)
#if defined(ART_DEBUG_TIMELINE) && defined(ART_TIMELINE_RECORDS_HERE)

// One record of eight 64-bit words per work item (slot = the item's number; items beyond kTimelineSlots are not recorded):
//   [0] XCC_ID << 32 | HW_ID;  [1..6] real-time clock (100 MHz) at the phase boundaries;  [7] shader clocks of the item.
// The lean forward item uses [3] = un-park events << 32 | stray rays, [4] = npass << 40 | tw << 20 | th, [5] = shader clocks and
// [7] = real-time clock at the start of the first flush (tools/timeline_report.py, tools/timeline_lean_report.py).
// The lean backward item stamps [5] at the end of its edge partition, BEFORE [3] and [4] (the end of the staging).
constexpr int kTimelineSlots = 16384;
static __device__ unsigned long long g_timeline[8 * kTimelineSlots];

struct Timeline {
    int slot;
    unsigned long long clk0;

    __device__ __forceinline__ bool writes() const { return threadIdx.x == 0 && (unsigned)slot < (unsigned)kTimelineSlots; }
    __device__ __forceinline__ void put(int k, unsigned long long v) const { if (writes()) g_timeline[8 * slot + k] = v; }
    // start of an item: the hardware id word, stamp 1, and the shader clock the span is measured from
    __device__ __forceinline__ void begin(int item_slot)
    {
        slot = item_slot;
        put(0, ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |     // XCC_ID
                   (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4));                    // HW_ID
        mark(1);
        clk0 = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void mark(int k) const { put(k, __builtin_amdgcn_s_memrealtime()); }
    // stamp k once this thread's outstanding loads have landed (the first traced group of the generic forward item)
    __device__ __forceinline__ void mark_landed(bool here, int k) const
    {
        if (here) { asm volatile("s_waitcnt vmcnt(0)"); mark(k); }
    }
    __device__ __forceinline__ void span(int k) const { put(k, __builtin_amdgcn_s_memtime() - clk0); }

    // The lean forward item: its window, and its stray rays / un-park events.  The two counters live in LDS and count_strays is
    // a STATIC member: it is called inside the ray lambda, where naming `tl` would add a capture - and with it another closure
    // layout and another register allocation - to the product build as well.
    static __device__ __forceinline__ unsigned* counters() { __shared__ unsigned s_dbg[2]; return s_dbg; }
    __device__ __forceinline__ void window(int npass, int tw, int th) const      // workgroup-uniform: holds a barrier
    {
        put(4, ((unsigned long long)npass << 40) | ((unsigned long long)tw << 20) | (unsigned)th);
        if (threadIdx.x < 2) counters()[threadIdx.x] = 0u;
        __syncthreads();
    }
    static __device__ __forceinline__ void count_strays(unsigned long long m_out, unsigned long long m_parked)
    {
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&counters()[0], (unsigned)__popcll(m_out));
            if (m_out & m_parked) atomicAdd(&counters()[1], 1u);
        }
    }
    __device__ __forceinline__ void end_lean(int k_counts, int k_span) const      // after the item's last barrier
    {
        put(k_counts, ((unsigned long long)counters()[1] << 32) | counters()[0]);
        span(k_span);
    }
};

// the last call's records -> the file named by the environment variable `env`: [items][8] u64, raw
static inline hipError_t dump_timeline(const char* env, int64_t items, hipStream_t stream)
{
    const char* out = getenv(env);
    if (out == nullptr) return hipSuccess;
    const int64_t n = std::min<int64_t>(items, kTimelineSlots);
    if (n <= 0) return hipSuccess;
    std::vector<unsigned long long> host(8 * n);
    hipError_t rc = hipStreamSynchronize(stream);
    if (rc == hipSuccess) rc = hipMemcpyFromSymbol(host.data(), HIP_SYMBOL(g_timeline), sizeof(unsigned long long) * 8 * n);
    if (rc != hipSuccess) return rc;
    if (FILE* f = fopen(out, "wb")) { fwrite(host.data(), sizeof(unsigned long long), host.size(), f); fclose(f); }
    return hipSuccess;
}

#else

struct Timeline {
    __device__ __forceinline__ void begin(int) {}
    __device__ __forceinline__ void mark(int) const {}
    __device__ __forceinline__ void mark_landed(bool, int) const {}
    __device__ __forceinline__ void span(int) const {}
    __device__ __forceinline__ void window(int, int, int) const {}
    static __device__ __forceinline__ void count_strays(unsigned long long, unsigned long long) {}
    __device__ __forceinline__ void end_lean(int, int) const {}
};
static inline hipError_t dump_timeline(const char*, int64_t, hipStream_t) { return hipSuccess; }

#endif

}  // namespace diag
}  // namespace art
