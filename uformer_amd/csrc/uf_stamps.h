// In-kernel instrumentation of the fused kernels behind ONE switch, UF_STAMPS (default 0).
//
// The shipped library is built with UF_STAMPS = 0: Census, LapTimer and stamp_now() are empty, no kernel reads the cycle counter
// or its tbuf parameter, and uf_debug_set_tbuf refuses a buffer (UF_ERR_UNSUPPORTED).  A counter read is a scalar memory
// operation: it costs ~40 cycles, sits on the critical path of the barrier it brackets, and leaves the scalar-memory counter
// "maybe pending", which turns the next counted LDS wait of the wave into a full one -- work the result never needs.
// The diagnostic library (scripts/build_variant.sh --stamps, -DUF_STAMPS=1) compiles the instrumentation in; scripts/ubench.py
// loads it through UFORMER_HIP_LIB for its stamp and census commands.  Every use in a kernel is either a member of the types
// below or sits under `if constexpr (UF_STAMPS != 0)`.
//
// This is the one preprocessor switch of the directory, and it is not an experiment knob (tests/test_host_logic.py keeps those out: an
// experiment lives in an A/B copy and only the winner lands).  The shipped arm comes first, the instrumented arm is the `#else`;
// tests/test_stamps_off.py checks that no clock is read anywhere outside that arm.
#pragma once
#include <hip/hip_runtime.h>

#if !defined(UF_STAMPS)
#define UF_STAMPS 0
#endif

namespace uf {

#if !UF_STAMPS
__device__ __forceinline__ unsigned long long stamp_now() { return 0; }
struct Census {
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void end(unsigned long long*, unsigned, bool) const {}
    __device__ __forceinline__ void end(unsigned long long*, unsigned) const {}
};
template <int N> struct LapTimer {
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void lap(int) {}
    __device__ __forceinline__ unsigned long long total(int) const { return 0; }
};
#else   // UF_STAMPS: the diagnostic build -- the only place in this directory that reads a clock
// the shader cycle counter (s_memtime)
__device__ __forceinline__ unsigned long long stamp_now() { return __builtin_readcyclecounter(); }

// debug census (uf_debug_set_tbuf): every workgroup records where and when it ran, so the host can count how many
// workgroups a CU really held at once and the effective shader clock.  Entry b at tbuf[65536 + 8 b]:
// {s_memtime start, end, wall_clock64 (100 MHz) start, end, HW_ID | XCC_ID << 32}.
struct Census {
    unsigned long long t0, r0;
    __device__ __forceinline__ void begin() { t0 = __builtin_readcyclecounter(); r0 = wall_clock64(); }
    // `writer`: the one thread of the workgroup that stores the entry
    __device__ __forceinline__ void end(unsigned long long* tbuf, unsigned block, bool writer) const {
        if (!tbuf || !writer) return;
        unsigned long long* o = tbuf + 65536 + (size_t)block * 8;
        o[0] = t0; o[1] = __builtin_readcyclecounter(); o[2] = r0; o[3] = wall_clock64();
        o[4] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
    }
    __device__ __forceinline__ void end(unsigned long long* tbuf, unsigned block) const { end(tbuf, block, threadIdx.x == 0); }
};

// N running totals of the cycles between consecutive lap() calls of a wave: lap(k) adds the time since the previous lap (or start) to total k
template <int N> struct LapTimer {
    unsigned long long t0, tot[N];
    __device__ __forceinline__ void start() {
#pragma unroll
        for (int k = 0; k < N; ++k) tot[k] = 0;
        t0 = __builtin_readcyclecounter();
    }
    __device__ __forceinline__ void lap(int k) { const unsigned long long t1 = __builtin_readcyclecounter(); tot[k] += t1 - t0; t0 = t1; }
    __device__ __forceinline__ unsigned long long total(int k) const { return tot[k]; }
};
#endif  // UF_STAMPS

}  // namespace uf
